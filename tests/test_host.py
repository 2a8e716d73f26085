"""CPU: host logic around the engine — parameter validation, device checks (the product path
refuses CPU tensors and has no CPU fallback), shard partitioning."""
import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import engine, sharding
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd._native import NativeLibraryError
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import risk_metrics
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams


def test_risk_params_validation():
    RiskParams().validate()
    with pytest.raises(ValueError):
        RiskParams(alpha=0.0).validate()
    with pytest.raises(ValueError):
        RiskParams(delta=float("inf")).validate()


def test_engine_refuses_cpu_tensors():
    s = torch.zeros((1, 2, 10, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        engine.safe_halfspaces(s, torch.zeros((2, 2), dtype=torch.float64))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu():
    with pytest.raises(NativeLibraryError):
        risk_metrics.device()
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import halfspaces
    with pytest.raises(NativeLibraryError):
        halfspaces.compute_safe_halfspaces([np.zeros((5, 2))], np.zeros(2), 0.3, 0.3, 0.2, 0.1, 0.15)


def test_risk_metric_kind():
    with pytest.raises(ValueError):
        risk_metrics.RiskMetric("var")
    assert risk_metrics.RiskMetric("cvar").params.alpha == 0.2


@pytest.mark.parametrize("units,world", [(0, 2), (1, 2), (7, 2), (200, 8), (1920, 8), (12800, 8), (5, 8)])
def test_shard_bounds_partition(units, world):
    spans = [sharding.shard_bounds(units, world, r) for r in range(world)]
    covered = []
    for a, b in spans:
        assert 0 <= a <= b <= units
        covered.extend(range(a, b))
    assert covered == list(range(units))
    per = -(-units // world) if units else 0
    assert all(b - a <= per for a, b in spans)


@pytest.mark.parametrize("O,T,world", [(3, 5, 4), (1, 7, 3), (4, 4, 2), (2, 3, 8), (5, 1, 2), (256, 50, 8)])
def test_shard_views_are_views_and_map_units(O, T, world):
    """Each rank's block is at most three strided views of the global tensor (never a copy, even
    for the reference's permuted [O, N, T, 2] order) and covers exactly units [start, stop)."""
    N = 3
    base = torch.arange(O * T * N * 2, dtype=torch.float64)
    layouts = [base.reshape(O, T, N, 2), base.reshape(O, N, T, 2).permute(0, 2, 1, 3)]
    ego = torch.arange(T * 2, dtype=torch.float64).reshape(T, 2)
    for s in layouts:
        seen = []
        for r in range(world):
            views, a, b = sharding.shard_views(s, ego, world, r)
            assert len(views) <= 3
            assert sum(c for *_, c in views) == b - a
            for sv, ev, off, cnt in views:
                assert sv.untyped_storage().data_ptr() == s.untyped_storage().data_ptr()
                o_n, t_n = sv.shape[:2]
                assert o_n * t_n == cnt and sv.shape[2:] == (N, 2)
                for k in range(cnt):
                    u = a + off + k
                    assert torch.equal(sv[k // t_n, k % t_n], s[u // T, u % T])
                    assert torch.equal(ev[k % t_n], ego[u % T])
                    seen.append(u)
        assert seen == list(range(O * T))


def test_shard_pieces_rejects_bad_blocks():
    with pytest.raises(ValueError):
        sharding.shard_pieces(2, 3, 4, 7)
    assert sharding.shard_pieces(2, 3, 2, 2) == []
    assert sharding.shard_pieces(4, 5, 3, 17) == [(0, 1, 3, 5, 0), (1, 3, 0, 5, 2), (3, 4, 0, 2, 12)]


def test_cluster_failure_retry_path(monkeypatch):
    """problems that end CLUSTER_TIMEOUT / CLUSTER_DIVERGED are re-solved on one
    workgroup each (options.cluster_size = 1) and patched into the batch result, with a warning."""
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import mpc_filter as mf
    B, O, H, nx, nu = 4, 3, 5, 4, 2
    hs_h, hs_g = torch.zeros(B, O, H, 2, dtype=torch.float64), torch.zeros(B, O, H, dtype=torch.float64)
    x0, xr, uf = torch.zeros(B, nx, dtype=torch.float64), torch.zeros(B, H + 1, nx, dtype=torch.float64), \
        torch.zeros(B, H, nu, dtype=torch.float64)
    x = torch.zeros(B, H + 1, nx, dtype=torch.float64)
    u = torch.zeros(B, H, nu, dtype=torch.float64)
    info = torch.zeros(B, _native.MPC_INFO_WIDTH, dtype=torch.float64)
    info[1, 0] = _native.MPC_STATUS_CLUSTER_TIMEOUT
    info[3, 0] = _native.MPC_STATUS_CLUSTER_DIVERGED
    info[2, 0] = _native.MPC_STATUS_NUMERICAL          # not a cluster failure: left alone
    calls = []

    def fake(model, h, g, x0_, xr_, uf_, max_iter, tol, polish, stream=None, options=None):
        calls.append((h.shape[0], options.cluster_size))
        n = h.shape[0]
        inf = torch.zeros(n, _native.MPC_INFO_WIDTH, dtype=torch.float64)
        inf[:, 1] = 7
        return (torch.full((n, H + 1, nx), 1.0, dtype=torch.float64),
                torch.full((n, H, nu), 2.0, dtype=torch.float64), inf)

    monkeypatch.setattr(mf, "filter_batch", fake)
    with pytest.warns(RuntimeWarning, match="re-solving"):
        got = mf.retry_cluster_failures(None, hs_h, hs_g, x0, xr, uf, x, u, info)
    assert got == [1, 3] and calls == [(2, 1)]
    assert torch.all(u[[1, 3]] == 2.0) and torch.all(u[[0, 2]] == 0.0)
    assert info[1, 0] == 0 and info[3, 1] == 7 and info[2, 0] == _native.MPC_STATUS_NUMERICAL
    calls.clear()
    assert mf.retry_cluster_failures(None, hs_h, hs_g, x0, xr, uf, x, u, info) == [] and calls == []


def test_stall_hook_rejects_output_group():
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import mpc_filter as mf
    with pytest.raises(ValueError):
        mf.make_options(debug_stall_group=0)
    assert mf.make_options(debug_stall_group=2).debug_stall_group == 3


def test_product_loader_reads_no_environment():
    """The library path is fixed unless use_library() is called (VERDICT r3 hygiene): the loader's
    source reads no environment variable."""
    import inspect
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
    src = inspect.getsource(_native)
    assert "os.environ" not in src and "getenv" not in src
    assert _native.LIB_PATH.endswith("_lib/libdrcvar_halfspace.so")


def test_profile_evidence_key_covers_the_unit_and_its_includes():
    """bench.py's roofline uses committed kernel-time evidence only while _native.source_key()
    matches: the key hashes the halfspace unit, the headers and the selection toolkit it includes,
    the toolchain and its flags -- not the MPC or sampler headers nor the generator, whose edits do
    not change the halfspace kernel."""
    import os
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
    src = os.path.join(_native.PKG_DIR, "csrc", "drcvar_halfspace.hip")
    incs = [os.path.basename(f) for f in _native._quoted_includes(src)]
    assert incs == ["drcvar_exchange.h", "drcvar_halfspace.h", "drcvar_selection.inc"]
    assert "drcvar_generator.inc" not in incs
    sampled = os.path.join(_native.PKG_DIR, "csrc", "drcvar_sampled.hip")
    sampled_incs = [os.path.basename(f) for f in _native._quoted_includes(sampled)]
    assert {"drcvar_generator.inc", "drcvar_selection.inc"} <= set(sampled_incs)
    assert _native.source_key() == _native.source_key("drcvar_halfspace.hip")
    assert _native.source_key("drcvar_mpc.hip") != _native.source_key()


def test_shared_kernel_helpers_are_defined_once():
    """The selection toolkit (drcvar_selection.inc) and the generator glue (drcvar_generator.inc)
    are shared by inclusion: a fix to the ranking or the bucket map is made in one place.  Each of
    these helpers is defined in exactly one file under csrc/."""
    import glob
    import os
    import re
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
    files = sorted(glob.glob(os.path.join(_native.PKG_DIR, "csrc", "*")))
    text = {os.path.basename(f): open(f).read() for f in files}
    assert "drcvar_selection.inc" in text and "drcvar_generator.inc" in text
    functions = ["make_log_scale", "make_params", "normal_quantile", "draw_pair", "wave_reduce",
                 "scan_loaded_bins", "rank_candidates_q", "f64_key"]
    # a definition: the name, its parameter list, then the opening brace (a call ends in ; or ,)
    patterns = {n: rf"\b{n}\s*\([^;{{}}]*\)\s*(const\s*)?\{{" for n in functions}
    patterns["struct BucketMap"] = r"\bstruct\s+BucketMap\s*\{"
    for name, pat in patterns.items():
        owners = [f for f, s in text.items() for _ in re.finditer(pat, s)]
        assert len(owners) == 1, (name, owners)
