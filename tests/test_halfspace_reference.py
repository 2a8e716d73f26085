"""CPU: the helper of the halfspace selection tests, pinned before the kernel is compared with it.

* the long-double reference (tests/halfspace_reference.py) against the NumPy closed form, the C
  oracle and the HiGHS restatement of the LPs, sentinel and NaN positions included;
* sensitivity: on every size of every launch geometry, in every alpha class, each seeded mistake
  (tau from rank m - 1 / m + 1, a tail sample dropped, a tie counted below tau) moves g_cvar by at
  least 10 x the unit's error bound — so a comparison at the bound fails on it;
* path coverage: the window mirror certifies, per launch geometry, that the case table holds
  robustly predicted units of every way out of the kernel's fast path.
"""
import numpy as np
import pytest

import halfspace_reference as hr
from oracle import c_oracle
from oracle import closed_form as cf
from oracle import lp_highs

P = (hr.RR, hr.RO)
LAUNCH_FORMS = hr.GEOMETRIES + [("stream",)]


def _ordinary(rng, U, n):
    s = rng.normal(size=(U, n, 2)) * rng.uniform(0.05, 1.0, size=(U, 1, 1)) + rng.uniform(-2, 2, size=(U, 1, 2))
    return s, rng.uniform(-3, 3, size=(U, 2))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 129, 1000])
@pytest.mark.parametrize("alpha", [0.2, 0.37, 1.0])
def test_reference_matches_closed_form_and_c_oracle(n, alpha):
    rng = np.random.default_rng(n)
    s, ego = _ordinary(rng, 6, n)
    ref = hr.reference(s, ego=ego, alpha=alpha)
    want = cf.safe_halfspaces(s[None], ego, *P, alpha, hr.DELTA, hr.EPSILON)[0]
    np.testing.assert_allclose(ref.rec, want, rtol=0, atol=1e-13)
    want_c = c_oracle.safe_halfspaces(s[None], ego, *P, alpha, hr.DELTA, hr.EPSILON)[0]
    np.testing.assert_allclose(ref.rec, want_c, rtol=0, atol=1e-13)
    h = rng.normal(size=(6, 2)) * rng.uniform(0.5, 2.0, size=(6, 1))
    refh = hr.reference(s, h=h, alpha=alpha)
    gc, gs, gt = cf.offsets_given_h(s, h, alpha, hr.DELTA, hr.EPSILON, *P)
    np.testing.assert_allclose(refh.rec[:, 5:8], np.stack([gc, gs, gt], axis=1), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(refh.rec[:, 3:5], h)
    want_c = c_oracle.offsets_given_h(s, h, *P, alpha, hr.DELTA, hr.EPSILON)
    np.testing.assert_allclose(refh.rec[:, 5:8], want_c[:, 5:8], rtol=0, atol=1e-13)
    # the bound is a rounding bound, not a tolerance: far below what the old tests allowed
    assert np.all(ref.bound < 1e-13 * max(n, 10)) and np.all(ref.bound > 0)


@pytest.mark.parametrize("seed", range(4))
def test_reference_matches_highs(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 60))
    alpha, _ = hr.alpha_of(n, float(rng.choice(hr.A0[1:5])))
    s, _ = _ordinary(rng, 1, n)
    h = rng.normal(size=(1, 2))
    ref = hr.reference(s, h=h, alpha=alpha)
    g_cvar = lp_highs.solve_cvar_lp(s[0], h[0], alpha, hr.DELTA, *P)
    g_star, g_tilde = lp_highs.solve_dr_cvar_lp(s[0], h[0], alpha, hr.DELTA, hr.EPSILON, *P)
    np.testing.assert_allclose(ref.rec[0, 5:8], [g_cvar, g_star, g_tilde], rtol=0, atol=1e-9)


def test_reference_sentinels_and_nan_positions():
    rng = np.random.default_rng(5)
    s, ego = _ordinary(rng, 4, 50)
    s[1, 49, 1] = np.nan
    s[2, 7, 0] = np.inf
    s[3] = s[3, :1]                       # all equal ...
    ego[3] = s[3, 0]                      # ... and the ego on the mean: the [1, 0] direction
    for alpha, eps in [(0.2, hr.EPSILON), (1.5, hr.EPSILON), (0.2, -0.1)]:
        ref = hr.reference(s, ego=ego, alpha=alpha, epsilon=eps)
        want = cf.safe_halfspaces(s[None], ego, *P, alpha, hr.DELTA, eps)[0]
        np.testing.assert_array_equal(np.isnan(ref.rec), np.isnan(want))
        np.testing.assert_array_equal(ref.rec == hr.SENTINEL, want == hr.SENTINEL)
        np.testing.assert_allclose(ref.rec, want, rtol=0, atol=1e-13, equal_nan=True)
        np.testing.assert_array_equal(ref.ok, [alpha <= 1, False, False, alpha <= 1])
    np.testing.assert_array_equal(ref.rec[3, 3:5], [1.0, 0.0])


def _cells(form):
    if form == ("stream",):
        return [(n, hr.STREAM_BLOCK) for n in hr.STREAM_SIZES]
    return [(n, hr.head_of(form[0], form[1])) for n in hr.sizes_of(form[0], form[1])]


@pytest.mark.parametrize("form", LAUNCH_FORMS, ids=str)
def test_every_seeded_mistake_exceeds_ten_bounds(form):
    """No unit is left out: in every planted family tau is unique and each of rank m - 1, rank
    m + 1 (where the rank exists) and the dropped tail sample (where m >= 1) moves g_cvar by at
    least 10 bounds.  The tie families (round01, three_values, crowd_tau) are exempt from the rank
    mutations only — a neighbouring rank holds the same value there — and must show the dropped
    sample (where a sample lies strictly below tau) and the tie counted below tau (where tau is
    tied and the unit is not all one value) at the same factor.  geometric, all_equal,
    collinear_perp and novar_exact have no neighbour of tau a rank mistake could resolve (spacings
    down to 2^-899, or none at all); they test exactness of the fallbacks, not sensitivity.
    gauss_plain is the Gaussian without the planted gap (ratios down to 2, which is why the gap is
    planted): it is there for the sum over several candidates below tau, which the gap empties."""
    worst = {}
    for n, head in _cells(form):
        for ac in range(len(hr.A0)):
            blk = hr.cases(n, ac, 0, head)
            ref = hr.reference(blk["samples"], ego=blk["ego"], alpha=blk["alpha"])
            assert ref.m == blk["m"] and ref.ok.all()
            for i, name in enumerate(blk["names"]):
                where = f"{name} N={n} a0={hr.A0[ac]}"
                if name in hr.PLANTED:
                    assert ref.n_eq[i] == 1, where
                    kinds = ("rank_lo", "rank_hi", "drop")
                    applies = (ref.m >= 1, ref.m + 1 <= n - 1, ref.m >= 1)
                elif name in hr.TIES:
                    kinds = ("drop", "le")
                    applies = (ref.n_below[i] >= 1, 2 <= ref.n_eq[i] < n)
                else:
                    continue
                for kind, ap in zip(kinds, applies):
                    g = hr.mutated_g_cvar(ref, i, kind)
                    assert (g is not None) == bool(ap), (where, kind)
                    if g is None:
                        continue
                    ratio = abs(g - ref.rec[i, 5]) / ref.bound[i]
                    worst[kind] = min(worst.get(kind, np.inf), ratio)
                    assert ratio >= 10.0, (where, kind, ratio, ref.bound[i])
    print(f"{form}: smallest |mutated - reference| / bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


# why a launch form cannot reach a class (anything not named here must be reached)
UNREACHABLE = {
    (64, 2, 7): {hr.CROWDED: "N <= 128: a bucket cannot hold more than kCap = 128 samples"},
}
CLASSES = (hr.FAST, hr.BELOW, hr.ABOVE, hr.CROWDED, hr.NOVAR)


@pytest.mark.parametrize("geo", hr.GEOMETRIES, ids=str)
def test_case_table_reaches_every_path_class(geo):
    """Per launch geometry, over its sizes and the alpha classes: at least one robustly predicted
    unit of each of FAST, BELOW, ABOVE, NOVAR and (where N > 128 allows it) CROWDED; and the
    families built to leave the fast path are predicted to: crowd_tau where it holds more than
    128 ties (N >= 172), geometric where N >= 256 and tau is not the isolated maximum, head_equal
    where the equal head is the kernel's whole subsample (N >= 2 heads).  (The streaming kernel has
    no window: every unit goes through the refinement of select_exact.)"""
    block, per, log_nb = geo
    head = hr.head_of(block, per)
    reached = {c: [] for c in CLASSES}
    for n in hr.sizes_of(block, per):
        for ac in range(len(hr.A0)):
            blk = hr.cases(n, ac, 0, head)
            ref = hr.reference(blk["samples"], ego=blk["ego"], alpha=blk["alpha"])
            for i, name in enumerate(blk["names"]):
                paths = hr.predict_paths(blk["samples"][i], ref.rec[i, 3:5], blk["alpha"], block, per,
                                         log_nb)
                if len(paths) == 1 and hr.UNSURE not in paths:
                    reached[next(iter(paths))].append((name, n, hr.A0[ac]))
                must_leave = ((name == "crowd_tau" and n >= 172)
                              or (name == "geometric" and n >= 256 and ac < len(hr.A0) - 1)
                              or (name == "head_equal" and n >= 2 * head))
                if must_leave:
                    assert hr.FAST not in paths and hr.UNSURE not in paths, (name, n, hr.A0[ac], paths)
    for c in CLASSES:
        why = UNREACHABLE.get(geo, {}).get(c)
        if why is not None:
            assert not reached[c], f"{geo} reaches {c} after all: drop it from UNREACHABLE ({why})"
        else:
            assert reached[c], f"{geo}: no robustly predicted {c} unit"
    print(f"{geo}: " + ", ".join(f"{c} {len(v)} ({sorted({x[0] for x in v})[:4]})" for c, v in reached.items()))


def test_window_mirror_restates_make_params():
    """z_alpha, the window and the rank as the kernel's host code sets them, at the alphas where
    the Acklam approximation changes branch."""
    for alpha, z in [(0.5, 0.0), (0.2, -0.8416212335729143), (0.02425, -1.9729), (0.001, -3.0902)]:
        assert abs(hr.normal_quantile(alpha) - z) < 2e-4
    z_lo, wsd, rank = hr.window_params(0.2, 10000)
    assert wsd == 0.25 and rank == 2000 and abs(z_lo - (-0.8416212335729143 - 0.25)) < 1e-8
    z_lo, wsd, rank = hr.window_params(0.2, 128)
    assert abs(wsd - 12 * np.sqrt(0.16 / 128) / (np.exp(-0.5 * 0.8416212335729143 ** 2) * 0.3989422804014327)) < 1e-7
    assert hr.window_params(1.0, 7)[2] == 6 and hr.window_params(0.01, 7)[2] == 0
