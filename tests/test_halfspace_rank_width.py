"""The express ranking of the fused halfspace kernel at every width of the target bucket, in both
forms of the small plans.

`rank_candidates_express_tail` visits the first candidate of a bucket in straight-line code beside
the tail's wave reduction and the rest in a loop (a build that visited four in straight-line code
was measured with this test and not kept, docs/lab_notebook.md section 4); the host runs a launch
of no more units than the device has compute units in the LONE form (candidate stores under a
narrowed exec mask) and every other launch in the SHARED form.  tests/rank_width_cases.py plants
buckets of c in {1, 2, 3, 4, 5, 6, 8, E, E + 1} candidates on the four small plans, with the wanted
rank first, second, last but one and last, with ties, and with the candidates in one wave or
spread over the waves.

The first test needs no GPU: the CPU restatement of the window certifies that every unit's bucket
holds exactly the c it planted and that tau one rank off moves g_cvar by at least 30 bounds.  The
GPU tests run every batch in chunks of at most 16 units, each chunk twice — alone (LONE) and as the
first units of a launch of CU count + 8 units (SHARED) — through the ego and the given-h entry:
records within the long-double reference's derived per-unit bound, and the two runs bitwise equal.
"""
import numpy as np
import pytest
import torch

import halfspace_reference as hr
import rank_width_cases as rw

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402

DEV = torch.device("cuda", 0)
CHUNK = 16
FORMS = ("ego", "given_h")


@pytest.mark.parametrize("plan", range(len(rw.PLANS)), ids=rw.IDS)
def test_buckets_hold_the_planted_counts(plan):
    """CPU: every unit realises its c, no (c, rank position, tie) that the plan can hold is
    missing, both placements occur, and a rank off by one is at least 30 bounds away."""
    (block, per, log_nb), n = rw.PLANS[plan]
    b = rw.batch(plan)
    e = 64 // (block // 64)
    for pts, c, label in zip(b["samples"], b["c"], b["labels"]):
        assert rw.bucket_count(pts, b["alpha"], block, per, log_nb) == c, label
    assert sorted(set(b["c"].tolist())) == rw.bucket_sizes(block) == sorted(
        {1, 2, 3, 4, 5, 6, 8, e, e + 1})
    for c in rw.bucket_sizes(block):
        mine = [lb for lb, cc in zip(b["labels"], b["c"]) if cc == c]
        have = {rw._position(r, c) for r in rw.RANKPOS for lb in mine if f"-{r}-" in lb}
        want = {p for p in (0, 1, c - 2, c - 1) if 0 <= p < c}
        if c == e + 1 and n - b["m"] < c:
            want.discard(0)                             # (the bucket would end past sample N - 1)
        assert have >= want, (rw.IDS[plan], c, have)
        ties = ["distinct"] + (["all_equal", "tau_twice"] if c >= 2 else []) + (
            ["tau_four_times"] if c >= 4 else [])
        for tie in ties:
            assert any(f"-{tie}-" in lb for lb in mine), (rw.IDS[plan], c, tie)
        if c >= 2:
            for placement in rw.PLACEMENTS:
                assert any(lb.endswith(placement) for lb in mine), (rw.IDS[plan], c, placement)
    for form in FORMS:
        ref = rw.reference(plan, form)
        assert ref.ok.all()
        # the candidates are the samples within the cluster's span of tau, and tau is of them
        ds = ref.d_sorted.astype(np.float64)
        near = (np.abs(ds - ds[:, [b["m"]]]) <= rw.SPACING * (b["c"][:, None] + 0.5)).sum(axis=1)
        assert (near == b["c"]).all()
        for i, label in enumerate(b["labels"]):
            for kind in ("rank_lo", "rank_hi"):
                j = b["m"] + (-1 if kind == "rank_lo" else 1)
                if ref.d_sorted[i, j] == ref.tau[i]:
                    continue                            # a tie: either rank gives the same value
                g = hr.mutated_g_cvar(ref, i, kind)
                gap = abs(g - ref.rec[i, 5]) / ref.bound[i]
                assert gap >= rw.MIN_GAP_BOUNDS, (rw.IDS[plan], form, label, kind, gap)


def _params(alpha):
    return RiskParams(hr.RR, hr.RO, alpha, hr.DELTA, hr.EPSILON)


def _launch(form, samples, alpha):
    """One launch over samples [U, N, 2] (numpy) -> (records [U, 8], status [U]) on the device."""
    s = torch.as_tensor(samples).to(DEV)
    u = s.shape[0]
    status = torch.full((u,), -1, dtype=torch.int32, device=DEV)
    if form == "given_h":
        h = torch.tensor([[1.0, 0.0]], dtype=torch.float64).repeat(u, 1).to(DEV)
        out = engine.offsets_given_h(s, h, _params(alpha), status=status)
    else:   # one obstacle, the units along the steps: one ego per unit
        e = torch.as_tensor(rw.ego_of(samples)).to(DEV)
        out = engine.safe_halfspaces(s[None], e, _params(alpha), status=status)[0]
    torch.cuda.synchronize()
    return out, status


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("plan", range(len(rw.PLANS)), ids=rw.IDS)
def test_every_bucket_width_in_both_forms(plan, form):
    (block, per, log_nb), n = rw.PLANS[plan]
    b, ref = rw.batch(plan), rw.reference(plan, form)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    big = cus + 8
    # these plans hold <= 8 samples per thread, so a launch of <= cus units takes the LONE form and
    # one of cus + 8 units the SHARED one: the rule is tested in tests/test_halfspace_form_host.py,
    # the form each such launch runs is observed in tests/test_halfspace_form_observed.py
    assert _native.launch_plan(n)[:2] == (block, per) and per <= 8 and CHUNK <= cus < big
    tol = np.stack([ref.bound_hm, ref.bound_hm, ref.bound_gm, ref.bound_h, ref.bound_h,
                    ref.bound, ref.bound, ref.bound], axis=1)
    if form == "given_h":
        tol[:, 0:5] = 1e-12
    worst = 0.0
    for lo in range(0, len(b["samples"]), CHUNK):
        chunk = b["samples"][lo:lo + CHUNK]
        u = len(chunk)
        lone, st_lone = _launch(form, chunk, b["alpha"])
        filler = chunk[np.arange(big - u) % u]
        shared, st_shared = _launch(form, np.concatenate([chunk, filler]), b["alpha"])
        assert (st_lone.cpu().numpy() == _native.UNIT_OK).all()
        assert (st_shared.cpu().numpy() == _native.UNIT_OK).all()
        got = lone.cpu().numpy()
        err = np.abs(got - ref.rec[lo:lo + u])
        ratio = err / tol[lo:lo + u]
        worst = max(worst, float(ratio[:, 5:8].max()))
        bad = np.argwhere(ratio > 1.0)
        assert bad.size == 0, [(b["labels"][lo + i], int(j), got[i, j], ref.rec[lo + i, j],
                                tol[lo + i, j]) for i, j in bad[:6]]
        same = torch.equal(lone, shared[:u])
        assert same, [b["labels"][lo + i] for i in
                      torch.nonzero((lone != shared[:u]).any(dim=1))[:6, 0].tolist()]
    print(f"RATIO {rw.IDS[plan]} {form} max error / bound {worst:.3f}, {len(b['samples'])} units")
