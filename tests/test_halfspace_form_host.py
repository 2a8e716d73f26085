"""CPU: the host's rule for the form of the halfspace kernel (the host-plans section of
csrc/drcvar_halfspace.hip: lone_capable, lone_form, halfspace_form), compiled into a stand-alone
program with the host compiler — the file itself, included with -DDRCVAR_HOST_PLANS_ONLY, which
leaves only that section: the same text the library's dispatch is compiled from.  LONE for the plans that hold at most 8
samples per thread when the launch has no more units than the device has compute units, SHARED
otherwise; the streaming kernel and the peer form never LONE; invalid arguments rejected with the
codes of include/drcvar_halfspace.h."""
import functools
import os
import shutil
import subprocess

import pytest

from conftest import REPO
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native

CSRC = os.path.join(REPO, "dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd", "csrc")
SHARED, LONE = 0, 1
PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "drcvar_halfspace.h"
namespace {
#define DRCVAR_HOST_PLANS_ONLY 1
#include "drcvar_halfspace.hip"
}
static_assert(kFormShared == 0 && kFormLone == 1, "the forms' numbers");
// argv: triples n_samples n_units cu_count -> one line each: rc form per peer_form ("-7" = untouched)
int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const long long n = atoll(argv[i]), units = atoll(argv[i + 1]), cus = atoll(argv[i + 2]);
    int32_t form = -7;
    const int rc = halfspace_form(n, units, static_cast<int32_t>(cus), &form);
    const int p = (n >= 1 && n <= DRCVAR_MAX_SAMPLES) ? pick_plan(n, 0, 0) : -1;
    const int per = p >= 0 ? kPlans[p].per : 0;
    const int peer = p >= 0 && lone_form(per, true, units, static_cast<int>(cus)) ? 1 : 0;
    printf("%d %d %d %d\n", rc, static_cast<int>(form), per, peer);
  }
  printf("null %d\n", halfspace_form(1000, 1, 256, nullptr));
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def program(tmp):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "hipcc")
                if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    src, exe = os.path.join(tmp, "form.cpp"), os.path.join(tmp, "form")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"), "-I", CSRC,
                    src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = program(str(tmp_path_factory.mktemp("form")))

    def run(*triples):
        """[(rc, form, per, peer_is_lone)] for (n_samples, n_units, cu_count) triples."""
        out = subprocess.run([exe] + [str(v) for t in triples for v in t], check=True,
                             capture_output=True, text=True).stdout.split("\n")
        assert out[len(triples)] == f"null {_native.ERR_INVALID_ARGUMENT}"
        return [tuple(int(v) for v in line.split()) for line in out[:len(triples)]]
    return run


@pytest.mark.parametrize("n", [100, 500, 1000, 2000])
def test_both_sides_of_the_threshold(ask, n):
    per = _native.launch_plan(n)[1]
    assert per <= 8
    for cus in (1, 80, 256, 304):
        got = ask((n, 1, cus), (n, cus, cus), (n, cus + 1, cus), (n, 100 * cus, cus))
        assert [g[:3] for g in got] == [(0, LONE, per), (0, LONE, per), (0, SHARED, per),
                                        (0, SHARED, per)], (n, cus, got)
        assert all(g[3] == 0 for g in got)              # the peer form has one form


def test_the_metric_shapes(ask):
    got = ask((1000, 80, 256), (1000, 200, 256), (1000, 264, 256), (1000, 128000, 256), (1000, 0, 256))
    assert [g[1] for g in got] == [LONE, LONE, SHARED, SHARED, SHARED]   # C2, C3, ..., C3 x 640, empty
    assert all(g[0] == 0 for g in got)


@pytest.mark.parametrize("n", [2049, 4096, 5000, 10000, _native.MAX_SAMPLES])
def test_large_plans_are_never_lone(ask, n):
    assert _native.launch_plan(n)[1] > 8
    got = ask((n, 1, 256), (n, 16, 256), (n, 256, 256))
    assert [g[:2] for g in got] == [(0, SHARED)] * 3 and got[0][2] == _native.launch_plan(n)[1]


@pytest.mark.parametrize("n", [_native.MAX_SAMPLES + 1, 40000, _native.MAX_SAMPLES_STREAM])
def test_the_streaming_kernel_is_never_lone(ask, n):
    assert _native.launch_plan(n)[1] == 0
    assert [g[:2] for g in ask((n, 1, 256), (n, 16, 256), (n, 256, 256))] == [(0, SHARED)] * 3


def test_rejects_invalid_arguments(ask):
    inv, uns = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED
    got = ask((0, 1, 256), (-5, 1, 256), (1000, -1, 256), (1000, 1, 0), (1000, 1, -3),
              (_native.MAX_SAMPLES_STREAM + 1, 1, 256))
    assert [g[:2] for g in got] == [(inv, -7)] * 5 + [(uns, -7)]       # form untouched when rejected


def test_the_plan_table_is_the_librarys(ask):
    """The included table answers as the loaded library's drcvar_launch_plan does."""
    sizes = [1, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 5120, 8192, 10240, 12288, 16384]
    got = ask(*[(n, 1, 256) for n in sizes])
    assert [g[2] for g in got] == [_native.launch_plan(n)[1] for n in sizes]
