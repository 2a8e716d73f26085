"""Records and status words of the selection tests' case tables, for a bit-for-bit comparison of
two builds of the engine (one library per process: DRCVAR_DIAG_LIB names a variant build).

    python scripts/micro/dump_selection_records.py OUT.npz
    python scripts/micro/dump_selection_records.py --compare A B     (.npz or .npy, each)

What is launched is what the tests launch, through their own helpers:
  stored    tests/test_halfspace_selection.py: the case block of tests/halfspace_reference.py at every
            size of every geometry (explicit plans through geometry=) and both streaming sizes, every
            alpha class, with ego and - on the automatic chain - with a given h (given_h_cases); the
            failure units of test_failure_words_every_form
  sampled   tests/test_sampled_halfspaces.py: the batches of test_fallback_and_ties on every plan and
            of test_failure_exits
--compare views every array as raw bytes, so NaNs count by bit pattern; exit status 1 on a difference.
"""
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import diaglib  # noqa: E402
diaglib.apply()  # DRCVAR_DIAG_LIB: a variant build (diagnostics)
import numpy as np  # noqa: E402


def load(path):
    a = np.load(path)
    return {"records": a} if isinstance(a, np.ndarray) else dict(a)


def compare(pa, pb):
    a, b = load(pa), load(pb)
    elements = differing = 0
    for key in sorted(set(a) | set(b)):
        if key not in a or key not in b or a[key].shape != b[key].shape or a[key].dtype != b[key].dtype:
            print(f"MISMATCH {key}: missing, or another shape or type")
            differing += 1
            continue
        x = np.ascontiguousarray(a[key]).view(np.uint8).reshape(a[key].shape + (-1,))
        y = np.ascontiguousarray(b[key]).view(np.uint8).reshape(b[key].shape + (-1,))
        d = int((x != y).any(axis=-1).sum())
        elements += a[key].size
        differing += d
        if d:
            print(f"DIFFERENT {key}: {d} of {a[key].size} elements")
    print(f"{pa} vs {pb}: {len(a)} arrays, {elements} elements, {differing} differ")
    return differing


def dump(out):
    import torch
    import halfspace_reference as hr
    import sampled_reference as sr
    import test_halfspace_selection as ts
    import test_sampled_halfspaces as tp
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native

    arrays = {}

    def put(key, rec, status):
        arrays[key + " rec"] = rec.cpu().numpy() if torch.is_tensor(rec) else rec
        arrays[key + " status"] = status.cpu().numpy() if torch.is_tensor(status) else status

    for form in ts.FORMS:
        geometry = None if form == ts.STREAM else form[:2]
        for n in ts._sizes(form):
            automatic = form == ts.STREAM or hr.automatic_geometry(n) == form
            for ac in range(ts.N_CLASSES):
                blk = hr.cases(n, ac, 0, ts._head(form))
                p = ts._params(blk["alpha"])
                put(f"safe {form} N={n} a0={ac}", *ts._run_safe(blk["samples"], blk["ego"], p, geometry))
                if automatic:
                    _, s, h = hr.given_h_cases(blk)
                    put(f"given-h {form} N={n} a0={ac}", *ts._run_given(s, h, p))
        n = ts._sizes(form)[0] if form == ts.STREAM else form[0] * (form[1] - 1) + 1
        _, s, ego, alpha = ts._failure_units(n, ts._head(form))
        h = hr.reference(s[:1], ego=ego[:1], alpha=alpha).rec[[0, 0, 0], 3:5]
        for a, eps in ((alpha, hr.EPSILON), (1.5, hr.EPSILON), (alpha, -0.1)):
            put(f"failure {form} N={n} alpha={a} eps={eps}", *ts._run_safe(s, ego, ts._params(a, eps), geometry))
            if form == ts.STREAM or hr.automatic_geometry(n) == form:
                put(f"failure given-h {form} N={n} alpha={a} eps={eps}", *ts._run_given(s, h, ts._params(a, eps)))
        print(f"stored {form}: {len(arrays)} arrays so far", flush=True)

    dev = torch.device("cuda", 0)
    for plan in sr.PLANS:
        n = sr.capacity(plan)
        for name, chol in list(tp.TIE_FACTORS.items()) + [("gauss", sr.factors_of(n)[0])]:
            for zero_first in ((True, False) if name == "sub_ulp" else (True,)):
                for a0 in hr.A0:
                    alpha, _ = hr.alpha_of(n, a0)
                    rec, st, _ = tp._run(dev, n, chol, alpha, zero_first_step=zero_first)
                    put(f"sampled {plan} {name} zf={zero_first} a0={a0}", rec, st)
        print(f"sampled {plan}: {len(arrays)} arrays so far", flush=True)
    nom, _, _ = tp._inputs(dev)
    for n in (100, 1000, 5001):
        for bad_u, coord in ((5, 0), (4, 1)):
            nan_nom = nom.clone()
            nan_nom.reshape(tp.U, 2)[bad_u, coord] = float("nan")
            rec, st, _ = tp._run(dev, n, sr.ISO, 0.2, nominal=nan_nom)
            put(f"sampled failure N={n} nan at {bad_u},{coord}", rec, st)
        for alpha, eps in ((0.2, hr.EPSILON), (1.5, hr.EPSILON), (0.2, -0.05), (1.5, -0.05)):
            rec, st, _ = tp._run(dev, n, sr.ISO, alpha, epsilon=eps)
            put(f"sampled failure N={n} alpha={alpha} eps={eps}", rec, st)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"wrote {out}: {len(arrays)} arrays from {_native._lib_path}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    dump(sys.argv[1])
