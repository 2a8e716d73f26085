"""GPU: a process whose very first launch of the engine happens inside a stream capture.

The launch code asks the device for its compute-unit count on first use (it chooses the form of
the small plans by it); that query must be legal under capture.  A fresh child process captures
its first launch (8 units, N = 1000) with torch.cuda.graph, replays the graph twice and compares
the records with an eager launch of the same batch."""
import os
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
if len(sys.argv) > 2 and sys.argv[2]:
    _native.use_library(sys.argv[2])
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(3)                 # drawn by torch: no engine launch yet
centre = torch.tensor([[[2.0, 1.0]], [[-1.5, 2.5]]], dtype=torch.float64, device=dev)
s = (0.2 * torch.randn((2, 4, 1000, 2), dtype=torch.float64, device=dev, generator=gen)
     + centre[:, :, None, :]).contiguous()                      # 8 units
e = torch.zeros((4, 2), dtype=torch.float64, device=dev)
out = torch.zeros((2, 4, engine.OUT_WIDTH), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
    launch, _ = engine.prepare_safe_halfspaces(s, e, RiskParams(), out=out,
                                               stream=torch.cuda.current_stream(dev))
    launch()                                                     # the process's first launch
replays = []
for _ in range(2):
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    replays.append(out.clone())
eager = engine.safe_halfspaces(s, e, RiskParams())
torch.cuda.synchronize()
assert torch.isfinite(eager).all() and (eager[..., 3:5].abs().sum(-1) > 0.5).all()
assert torch.equal(replays[0], eager) and torch.equal(replays[1], eager)
print("FIRST-LAUNCH-CAPTURED ok")
"""


def test_first_launch_inside_capture():
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, os.environ.get("DRCVAR_DIAG_LIB", "")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FIRST-LAUNCH-CAPTURED ok" in r.stdout
