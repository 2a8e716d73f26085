"""GPU: which form of the halfspace kernel a launch ran, observed — not restated.

A child process runs with the HIP runtime's launch log switched on (AMD_LOG_LEVEL=3: one
"ShaderName : ..." line per dispatch, with the kernel's template arguments, the last of which is
the LONE flag) and launches, on each small plan and through both entries, 16 units and CU count + 8
units; then 16 units on a large plan.  The parent reads the names: LONE for the small launches of
the small plans, SHARED for everything else.  A host that never chose LONE, or always did, fails
here; the records of the two forms are compared in tests/test_halfspace_rank_width.py."""
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
if sys.argv[2]:
    _native.use_library(sys.argv[2])
dev = torch.device("cuda", 0)
cus = torch.cuda.get_device_properties(dev).multi_processor_count
gen = torch.Generator(device=dev).manual_seed(1)
for n in (128, 512, 1000, 2000, 5000):
    for units in ((16, cus, cus + 8) if n <= 2000 else (16,)):
        s = (0.2 * torch.randn((1, units, n, 2), dtype=torch.float64, device=dev, generator=gen) + 2.0)
        e = torch.zeros((units, 2), dtype=torch.float64, device=dev)
        h = torch.tensor([[1.0, 0.0]], dtype=torch.float64, device=dev).repeat(units, 1)
        for entry in ("ego", "given_h"):
            torch.cuda.synchronize()
            sys.stderr.write(f"\nMARK {n} {units} {cus} {entry}\n")
            sys.stderr.flush()
            if entry == "ego":
                out = engine.safe_halfspaces(s, e, RiskParams())
            else:
                out = engine.offsets_given_h(s[0], h, RiskParams())
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
sys.stderr.write("\nMARK end\n")
"""


def test_the_form_each_launch_ran():
    env = dict(os.environ, AMD_LOG_LEVEL="3")
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, os.environ.get("DRCVAR_DIAG_LIB", "")],
                       capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = []
    for block in r.stderr.split("\nMARK ")[1:]:
        head = block.split("\n", 1)[0].split()
        if head[0] == "end":
            break
        n, units, cus, entry = int(head[0]), int(head[1]), int(head[2]), head[3]
        names = re.findall(r"ShaderName : .*?safe_halfspace_kernel<([^>]*)>", block)
        assert len(names) == 1, (head, names)           # one launch, one dispatch of the kernel
        args = [a.strip() for a in names[0].split(",")]
        assert len(args) == 8, args
        assert args[4] == ("true" if entry == "given_h" else "false"), (head, args)
        want = "true" if (n <= 2000 and units <= cus) else "false"
        assert args[7] == want, (head, args)
        seen.append((n, units, entry, args[7]))
    assert len(seen) == 2 * (4 * 3 + 1), seen
    assert {s[3] for s in seen} == {"true", "false"}
