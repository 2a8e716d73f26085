"""GPU: the peer record exchange (include/drcvar_exchange.h, sharding.PeerExchange), in both forms:
push (the kernel writes every record into every rank's region) and pull (into its own region; the
small launch copies every rank's rows from that rank's region).

Every step of every test here has records of its OWN: eager steps re-draw the rank's samples in
place (the sampler's `stream_offset` = the step index), captured steps shift the per-unit ego in
place inside the graph, `out` is NaN-filled before every step, and each step is compared bitwise
with the PLAIN launch (the one tests/test_gpu_parity.py holds against the oracle) of that step's
inputs.  A skipped wait, a read or write of the wrong parity buffer, or a stale read of a peer's
rows therefore returns rows of another step (or zeros, or NaN) and fails the comparison; that the
expected records do differ from step to step is itself asserted.

* one rank (the exchange with itself): ShardedBatch(exchange="peer") gives bitwise the records of
  the plain launch, step after step, eager and replayed from a hipGraph (three captured steps per
  replay, so a captured step's parity alternates between replays; each captured step's output is
  copied aside inside the graph and checked), the generation counts the steps, the error word stays
  0 and `check_exchange()` is silent;
* two and four processes on the one GPU of the box (gloo control group; each maps the others'
  regions by IPC — the same code path as xGMI peers, minus the link): every rank ends every step
  with the whole batch's records, bitwise, including steps where one rank is LATE (a calibrated
  >= 20 ms device delay ahead of its kernel, alternated so that each end is late at each parity):
  a wait that returned early would hand the punctual ranks the late rank's rows of two steps ago;
* a wait whose peer never signals gives up at its spin limit and sets the error word (bit 63 and
  the silent rank's bit) instead of hanging, and `PeerExchange.check()` raises, naming that rank;
* every one of the ten automatic launch plans runs in the peer form (one N per plan), plus the
  non-temporal load form on C5's plan (a 272 MB launch), on a crafted block (ordinary units, heavy
  ties, an all-equal unit, all-equal-but-the-pivot, a NaN sample) and with `alpha > 1` and
  `epsilon < 0`: bitwise the plain launch, the C oracle within the project's tolerances, and the
  same per-unit status words;
* `step()` issued while another stream is current still orders the publish/wait/copy behind its
  kernel (both go to the stream the launches were prepared on).

scripts/micro/patches/peer_fault_switches.diff seeds three faults (copy reads the other parity; no
wait; records stored into the other parity) as variant builds; docs/lab_notebook.md records which
of these tests fail on each.  Cross-DEVICE behaviour (xGMI, 8 ranks) is exercised only by the
driver's multi-GPU bench (bench.py strong_scaling, `exchanges.peer`, which checks its records
against the RCCL all-gather's before using it).
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine, sharding, synthetic
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SHIFT = (1.0 / 64, -1.0 / 128)     # the captured steps' per-step ego shift (exact in binary)
GRAPH_STEPS, REPLAYS = 3, 3        # an odd number of steps per replay: parities alternate
H_TOL, OFFSET_TOL = 1e-12, 1e-6    # tests/test_gpu_parity.py / conftest.py (the north star's)
DELAY_MIN_MS = 20.0                # a late rank is at least this late ...
DELAY_MAX_FRACTION = 0.1           # ... and at most this fraction of the wait's spin limit


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- step k's inputs and expected records -------------------------------------------------------

def _redraw(sb, nominal, N, seed, k):
    """Step k's samples of this rank's block, drawn in place (the frozen launch holds the pointer)."""
    obstacles.sample_units_device(nominal, N, sb.start, sb.count, seed=seed, stream_offset=k,
                                  out=sb.samples)


def _expected(nominal, ego, N, seed, k, params=RiskParams()):
    """Step k's whole batch and its records by the plain launch (tests/test_sampling.py: the unit
    range above is a slice of exactly this batch)."""
    s = obstacles.sample_trajectories_device(nominal, N, seed=seed, stream_offset=k)
    return s, engine.safe_halfspaces(s, ego, params)


def _delay(dev, spin_limit_us):
    """(enqueue, ms): a device delay on the current stream of >= DELAY_MIN_MS and <= a tenth of the
    spin limit, calibrated once with HIP events (torch.cuda._sleep, else a chain of matmuls)."""
    hi_ms = DELAY_MAX_FRACTION * spin_limit_us / 1000.0
    target = min(3.0 * DELAY_MIN_MS, 0.5 * (DELAY_MIN_MS + hi_ms))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    if hasattr(torch.cuda, "_sleep"):
        unit = lambda c: torch.cuda._sleep(int(c))                     # noqa: E731
        c = 1_000_000
    else:
        m = torch.randn((1024, 1024), device=dev)
        tmp = torch.empty_like(m)

        def unit(c):
            for _ in range(int(c)):
                torch.mm(m, m, out=tmp)
        c = 20
    unit(c)                                                            # warm-up (first launch)
    for _ in range(3):                                                 # scale towards the target
        c = max(1, int(c * target / max(timed(lambda: unit(c)), 1e-3)))
    ms = timed(lambda: unit(c))
    assert DELAY_MIN_MS <= ms <= hi_ms, f"calibrated delay {ms:.1f} ms outside [{DELAY_MIN_MS}, {hi_ms}] ms"
    return (lambda: unit(c)), ms


def _exercise(sb, nominal, ego, N, seed, dev, late, delay=None, barrier=None):
    """Eager steps (step k: samples re-drawn with stream_offset k; `late[k]` is the rank that is
    late at step k, or None), then GRAPH_STEPS captured steps replayed REPLAYS times (the ego
    shifted in place before each).  Every step: `out` NaN-filled before, records bitwise the plain
    launch's of that step's inputs after, expected records different from the previous step's,
    generation = steps so far, error word 0.  Returns the failures (strings); [] = all held.
    Failures are collected, not raised, so that the ranks of a multi-process run stay in step."""
    fails = []

    def expect(cond, what):
        if not cond:
            fails.append(what)

    def clean(steps, where):
        if sb.peer is not None:
            gen, err = sb.peer.generation(), sb.peer.error()
            expect(gen == steps and err == 0, f"{where}: generation {gen} (want {steps}), error {err:#x}")
        try:
            sb.check_exchange()
        except RuntimeError as exc:
            fails.append(f"{where}: check_exchange raised {exc}")

    O, T, U = sb.O, sb.T, sb.U
    steps, prev, whole = 0, None, None
    for k, who in enumerate(late):
        _redraw(sb, nominal, N, seed, k)
        whole, want = _expected(nominal, ego, N, seed, k)
        if prev is not None:   # (t = 0 is noise-free: the same samples at every step)
            expect(bool((want != prev).any(-1)[:, 1:].all()) and not torch.equal(want, prev),
                   f"eager step {k}: the expected records do not differ from step {k - 1}'s")
        sb.full.fill_(NAN)
        if who == sb.rank:
            delay()
        sb.step()
        torch.cuda.synchronize(dev)
        steps += 1
        where = f"eager step {k}" + ("" if who is None else f" (rank {who} late)")
        expect(torch.equal(sb.records(), want), f"{where}: records differ from the plain launch's")
        clean(steps, where)
        prev = want
    # graph capture and replay (the bench's form): the parity comes from the device counter
    shift = torch.tensor(SHIFT, dtype=torch.float64, device=dev)
    ego_all = ego.index_select(0, torch.arange(U, device=dev) % T).contiguous()   # every rank's units
    flat = whole.view(1, U, N, 2)                     # the grid shape ShardedBatch itself uses
    snaps = torch.full((GRAPH_STEPS,) + tuple(sb.full.shape), NAN, dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        launch = sb.prepare(torch.cuda.current_stream(dev))
        for j in range(GRAPH_STEPS):
            sb.full.fill_(NAN)
            sb.ego_units.add_(shift)
            sb.step(launch)
            snaps[j].copy_(sb.full)
    if barrier is not None:
        barrier()
    for r in range(REPLAYS):
        snaps.fill_(NAN)
        sb.full.fill_(NAN)
        g.replay()
        torch.cuda.synchronize(dev)
        for j in range(GRAPH_STEPS):
            ego_all.add_(shift)       # the same adds of the same operands: the same bits
            want = engine.safe_halfspaces(flat, ego_all, RiskParams()).view(O, T, engine.OUT_WIDTH)
            where = f"replay {r}, captured step {j}"
            expect(bool((want != prev).any(-1).all()),
                   f"{where}: some unit's expected record does not differ from the step before")
            expect(torch.equal(snaps[j][:U].view(O, T, engine.OUT_WIDTH), want),
                   f"{where}: records differ from the plain launch's")
            prev = want
        steps += GRAPH_STEPS
        expect(torch.equal(sb.records(), prev), f"replay {r}: records() is not the last captured step's")
        clean(steps, f"replay {r}")
    return fails, steps


@pytest.mark.parametrize("form", ["peer", "peer_pull"])
@pytest.mark.parametrize("O,T,N", [(10, 20, 1000), (7, 9, 300), (3, 5, 5000)])
def test_peer_exchange_one_rank_matches_plain_launch(dev, O, T, N, form):
    nominal, ego = synthetic.nominal_paths(O, T, dev, seed=5), synthetic.straight_line_ego(T, dev)
    sb = sharding.ShardedBatch(nominal, ego, N, RiskParams(), 1, 0, seed=5, exchange=form,
                               force_exchange=True)
    assert sb.peer is not None and sb.peer.rows == O * T
    # three eager steps: both parities, then the first again
    fails, steps = _exercise(sb, nominal, ego, N, 5, dev, late=[None] * 3)
    assert not fails, fails
    assert steps == 3 + GRAPH_STEPS * REPLAYS
    assert sb.peer.generation() == steps and sb.peer.error() == 0
    sb.close()


def _rank_worker(rank, world, port, O, T, N, q, form="peer"):
    import sys
    sys.path.insert(0, REPO)
    if os.environ.get("DRCVAR_DIAG_LIB"):     # a variant build (spawned: not through conftest.py)
        _native.use_library(os.environ["DRCVAR_DIAG_LIB"])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"rank": rank}
    try:
        nominal, ego = synthetic.nominal_paths(O, T, dev, seed=9), synthetic.straight_line_ego(T, dev)
        sb = sharding.ShardedBatch(nominal, ego, N, RiskParams(), world, rank, seed=9, exchange=form)
        delay, res["delay_ms"] = _delay(dev, sb.peer.spin_limit_us)
        # three punctual steps, then four with one rank late: each end late at each parity
        late = [None] * 3 + [0, world - 1, world - 1, 0]
        res["fails"], res["steps"] = _exercise(sb, nominal, ego, N, 9, dev, late, delay, dist.barrier)
        res["gen"], res["err"] = sb.peer.generation(), sb.peer.error()
        sb.close()
        # the failure path: only rank 0 signals and waits; its wait gives up at its spin limit
        px = sharding.PeerExchange(8, world, rank, dev, spin_limit_us=50_000,
                                   mode="pull" if form == "peer_pull" else "push")
        if rank == 0:
            px.signal_wait()
            torch.cuda.synchronize(dev)
        res["timeout_err"] = px.error()
        try:
            px.check()
            res["check"] = None
        except RuntimeError as exc:
            res["check"] = str(exc)
        px.close()
    except Exception as exc:  # noqa: BLE001 - reported to the parent
        res["exception"] = repr(exc)
    finally:
        q.put(res)
        dist.destroy_process_group()


def _run_ranks(world, O, T, N, form):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, O, T, N, q, form)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=240) for _ in procs), key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    silent = sum(1 << j for j in range(1, world))      # every rank but 0 stayed silent
    for res in results:
        rank = res["rank"]
        assert "exception" not in res, (rank, res["exception"])
        assert not res["fails"], (rank, res["fails"])
        assert DELAY_MIN_MS <= res["delay_ms"] <= 200.0, res["delay_ms"]
        assert res["steps"] == 7 + GRAPH_STEPS * REPLAYS
        assert res["gen"] == res["steps"] and res["err"] == 0, (rank, res["gen"], res["err"])
        if rank == 0:
            assert res["timeout_err"] == (1 << 63) | silent, hex(res["timeout_err"])
            assert res["check"] is not None, "rank 0's check() did not raise after its wait gave up"
            assert f"rank(s) {list(range(1, world))}" in res["check"], res["check"]
        else:
            assert res["timeout_err"] == 0
            assert res["check"] is None, res["check"]


@pytest.mark.parametrize("form", ["peer", "peer_pull"])
@pytest.mark.parametrize("O,T,N", [(10, 20, 1000), (5, 3, 64)])
def test_peer_exchange_two_processes_one_gpu(dev, O, T, N, form):
    _run_ranks(2, O, T, N, form)


@pytest.mark.parametrize("form", ["peer", "peer_pull"])
def test_peer_exchange_four_processes_one_gpu(dev, form):
    """15 units over 4 ranks: per = 4 and one padded row; lanes 0..3 of the record store, the pull
    form's search for the rank whose block holds a row."""
    _run_ranks(4, 5, 3, 64, form)


# ---- every instantiation of the peer form -------------------------------------------------------

PLAN_N = [100, 500, 1000, 2000, 4000, 5000, 8000, 10000, 12000, 16384]   # one per automatic plan
PARAM_CASES = ([(n, RiskParams()) for n in PLAN_N]
               + [(n, RiskParams(alpha=1.5)) for n in (1000, 10000)]      # every unit: failure exit
               + [(n, RiskParams(epsilon=-0.1)) for n in (1000, 10000)])  # g* = 100, g~ = 100 - R_c|h|


def test_peer_form_sizes_cover_every_plan(dev):
    plans = {_native.launch_plan(n)[:2] for n in PLAN_N}
    assert plans == {(64, 2), (128, 4), (256, 4), (256, 8), (256, 16), (256, 20), (512, 16), (512, 20),
                     (1024, 12), (1024, 16)}
    assert len(plans) == len(PLAN_N) == 10


def _crafted_block(N, seed):
    """[8, N, 2]: four ordinary units, heavy ties (the refinement path), all samples equal (the
    degenerate path), all equal but the pivot (sample 0), one NaN sample (solver failure)."""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(8, N, 2)) * 0.2 + rng.uniform(-3, 3, size=(8, 1, 2))
    b[4] = np.round(b[4], 1)
    b[5] = b[5, 0]
    b[6, 1:] = b[6, 1]
    b[6, 0] = b[6, 1] + (0.25, -0.5)
    b[7, N // 3, 0] = np.nan
    return b


def _assert_bitwise(got, want, what):
    """NaN in the same places; every other value the same bits."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(got.contiguous().view(torch.int64)[~nan], want.contiguous().view(torch.int64)[~nan]), what


def _assert_match(got, want):
    """tests/test_gpu_parity.py's rules against the oracle, restated."""
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    g, w = np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)
    np.testing.assert_allclose(g[..., [0, 1, 3, 4]], w[..., [0, 1, 3, 4]], rtol=0, atol=H_TOL)
    np.testing.assert_allclose(g[..., [2, 5, 6, 7]], w[..., [2, 5, 6, 7]], rtol=0, atol=OFFSET_TOL)
    np.testing.assert_array_equal(got[..., 5] == 100.0, want[..., 5] == 100.0)
    np.testing.assert_array_equal(got[..., 6] == 100.0, want[..., 6] == 100.0)


def _oracle(samples, ego, p, **kw):
    from oracle import c_oracle
    return c_oracle.safe_halfspaces(samples, ego, p.robot_radius, p.obstacle_radius, p.alpha, p.delta,
                                    p.epsilon, **kw)


@pytest.mark.parametrize("form", ["peer", "peer_pull"])
@pytest.mark.parametrize("N,params", PARAM_CASES,
                         ids=[f"N{n}-a{p.alpha}-e{p.epsilon}" for n, p in PARAM_CASES])
def test_peer_form_every_plan(dev, N, params, form):
    """One rank, 2 x 4 crafted units, two steps (one per parity; the second on another crafted
    block, through a launch that also asks for the status words): the peer form's records are
    bitwise the plain launch's, match the C oracle, and its status words are the plain launch's."""
    O, T = 2, 4
    host = [_crafted_block(N, 7 * N + i) for i in range(2)]
    ego_h = np.random.default_rng(N).uniform(-3, 3, size=(T, 2))
    ego = torch.as_tensor(ego_h).to(dev)
    nominal = torch.zeros((O, T, 2), dtype=torch.float64, device=dev)      # unused: samples are given
    block = torch.as_tensor(host[0]).to(dev)
    sb = sharding.ShardedBatch(nominal, ego, N, params, 1, 0, exchange=form, force_exchange=True,
                               samples=block)
    st_plain = torch.full((O, T), -1, dtype=torch.int32, device=dev)
    st_peer = torch.full((O * T,), -1, dtype=torch.int32, device=dev)
    with_status = sb.peer.prepare_launch(block.unsqueeze(0), sb.ego_units, params, 0, status=st_peer)
    prev = None
    for k in range(2):
        block.copy_(torch.as_tensor(host[k]))
        want = engine.safe_halfspaces(block.view(O, T, N, 2), ego, params, status=st_plain)
        sb.full.fill_(NAN)
        if k == 0:
            sb.step()                       # the status pointer NULL, as ShardedBatch launches it
        else:
            with_status()
            sb.exchange()
        torch.cuda.synchronize(dev)
        _assert_bitwise(sb.records(), want, f"step {k}")
        assert sb.peer.generation() == k + 1 and sb.peer.error() == 0
        sb.check_exchange()
        assert prev is None or not torch.equal(want.nan_to_num(7.0), prev.nan_to_num(7.0))
        prev = want
        if k == 0:
            _assert_match(sb.records().cpu().numpy(), _oracle(host[0].reshape(O, T, N, 2), ego_h, params))
    assert torch.equal(st_peer.view(O, T), st_plain), (st_peer.tolist(), st_plain.tolist())
    st, rec = st_plain.view(-1).tolist(), sb.records().view(O * T, 8).cpu().numpy()
    rch = (params.robot_radius + params.obstacle_radius) * np.hypot(rec[:7, 3], rec[:7, 4])
    if params.alpha > 1.0:                  # every unit takes the failure exit
        assert st[:7] == [_native.UNIT_UNBOUNDED] * 7 and st[7] & _native.UNIT_NONFINITE
        assert (rec[:, 5] == 100.0).all() and (rec[:, 6] == 100.0).all()
        np.testing.assert_allclose(rec[:7, 7], 100.0 - rch, rtol=0, atol=OFFSET_TOL)
    elif params.epsilon < 0.0:              # the DR offsets are the sentinel's, the CVaR offset stands
        assert st[:7] == [_native.UNIT_DR_UNBOUNDED] * 7 and st[7] & _native.UNIT_NONFINITE
        assert (rec[:, 6] == 100.0).all() and (rec[:7, 5] != 100.0).all()
        np.testing.assert_allclose(rec[:7, 7], 100.0 - rch, rtol=0, atol=OFFSET_TOL)
    else:
        assert st[:7] == [_native.UNIT_OK] * 7 and st[7] == _native.UNIT_NONFINITE
        assert (rec[:7, 5:] != 100.0).all() and rec[7, 5] == 100.0 and rec[7, 6] == 100.0
    sb.close()


@pytest.mark.parametrize("form", ["peer", "peer_pull"])
def test_peer_form_nontemporal_loads_on_c5_plan(dev, form):
    """N = 10 000 (plan 512 x 20, C5's) x 34 x 50 units = 272 MB, above the 256 MB from which a
    launch reads its samples with non-temporal loads: two steps (the ego shifted in between), each
    bitwise the plain launch of the same block (the same load form), the first against the C oracle
    on every 97th unit."""
    O, T, N = 34, 50, 10000
    assert O * T * N * 16 > 256 << 20 and _native.launch_plan(N)[:2] == (512, 20)
    nominal, ego = synthetic.nominal_paths(O, T, dev, seed=13), synthetic.straight_line_ego(T, dev)
    sb = sharding.ShardedBatch(nominal, ego, N, RiskParams(), 1, 0, seed=13, exchange=form,
                               force_exchange=True)
    ego_all = sb.ego_units.clone()
    shift = torch.tensor(SHIFT, dtype=torch.float64, device=dev)
    prev = None
    for k in range(2):
        if k:
            sb.ego_units.add_(shift)
            ego_all.add_(shift)
        want = engine.safe_halfspaces(sb.samples.unsqueeze(0), ego_all, RiskParams()).view(O, T, 8)
        sb.full.fill_(NAN)
        sb.step()
        torch.cuda.synchronize(dev)
        assert torch.equal(sb.records(), want), k
        assert sb.peer.generation() == k + 1 and sb.peer.error() == 0
        sb.check_exchange()
        assert prev is None or bool((want != prev).any(-1).all())
        prev = want
        if k == 0:
            sub = sb.samples[::97].cpu().numpy()[None]
            ref = _oracle(sub, ego_all[::97].cpu().numpy(), RiskParams(), nthreads=8)
            _assert_match(sb.records().view(O * T, 8)[::97].cpu().numpy()[None], ref)
            # the whole-batch grid [O, T] x ego [T, 2] takes the same load form and gives the same bits
            assert torch.equal(engine.safe_halfspaces(sb.samples.view(O, T, N, 2), ego, RiskParams()), want)
    sb.close()
    del sb, want, prev
    torch.cuda.empty_cache()


# ---- host side ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["peer", "peer_pull"])
def test_step_on_a_side_stream_stays_behind_its_kernel(dev, form):
    """The launches are frozen on the stream of construction; a step() issued while ANOTHER stream
    is current must put its publish/wait/copy on that same stream, behind the kernel — here the
    kernel is held back by a delay on the default stream, so a copy on the side stream would run
    first and return the rows the buffer held before."""
    O, T, N = 7, 9, 300
    nominal, ego = synthetic.nominal_paths(O, T, dev, seed=5), synthetic.straight_line_ego(T, dev)
    sb = sharding.ShardedBatch(nominal, ego, N, RiskParams(), 1, 0, seed=5, exchange=form,
                               force_exchange=True)
    sb.step()
    torch.cuda.synchronize(dev)
    _, want0 = _expected(nominal, ego, N, 5, 0)
    assert torch.equal(sb.records(), want0)
    _redraw(sb, nominal, N, 5, 1)
    _, want1 = _expected(nominal, ego, N, 5, 1)
    assert bool((want1 != want0).any(-1)[:, 1:].all())
    delay, _ = _delay(dev, sb.peer.spin_limit_us)
    side = torch.cuda.Stream(dev)
    sb.full.fill_(NAN)
    torch.cuda.synchronize(dev)
    delay()                                   # on the default stream, ahead of the kernel
    with torch.cuda.stream(side):
        sb.step()
    torch.cuda.synchronize()
    assert torch.equal(sb.records(), want1)
    assert sb.peer.generation() == 2 and sb.peer.error() == 0
    sb.check_exchange()
    sb.close()
