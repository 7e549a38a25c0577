"""The RANK FORM of skewed, decisions-only batches (csrc/range_part.hpp: k_tile_part<PART_RANK>, rs::k_finish's scan of the hot
ids' columns, ev::eval_hot_role) on streams whose hot keys are still ALLOWED: the partition leaves id << 16 | rank for every
request of a hot slot, the finish scans the tiles' counts into hot_P, and the hot role finds A = the allowed requests of a slot's
run by bisection and allows a request iff hot_P[tile][id] + rank < A; its last block stores cell_after(new0 + lo * inc).  The
streams of test_gpu_range.py and test_gpu_timed_config.py drain their hot keys before the form switches on (A = 0 from the second
batch on), so neither the bisection, nor the prefix across tiles, nor the stored cell was compared with anything there.

Entry into the form is made deterministic with switches the library has: TCGPU_HOT_THREAD=0 (the list is made on the caller's
thread) and a device synchronisation after every batch (the notes and hints of a batch are published when the next call looks).
Every batch's decision bytes, the counters, the resident state of every slot touched (in the middle and at the end) and the
engine's self check are compared bit for bit with the oracle applying the requests one by one; which batches took the form is
read from the engine, and what the form had to work out in them (partial allowances, runs that cross tiles) from the oracle."""
import numpy as np
import pytest

from tests.test_gpu_slots import T0, _oracle, assert_state_same

pytestmark = pytest.mark.gpu

HOT = "range path, hot slots peeled"
TILE = 4096                                                      # requests per tile of the partition (rp::PT_TILE)
STEPS_NS = (50_000_000, 5_000_000, 0, 20_000_000, -10_000_000)   # between batches; the negative one: request 0 of a drained run is denied
FAST = (3000, 60000, 1)                                          # ei = 16 666 ns, dvt ~ 50 ms: 3 000 tokens come back in 50 ms
# per-slot plans of case 2, tier = slot % 4: tokens that come back in (50, 5, 0, 20) ms -> (3000, 300, 0, 1200), (500, 100, 0, 400),
# (5, 1, 0, 4), (40, 5, 0, 20): the third one is where a run with exactly ONE allowed request comes from
TIERS = (FAST, (500, 20000, 1), (5, 200, 1), (40, 1000, 1))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _host(x):
    return x.cpu().numpy()


def _head(cap, k):
    """k hot slots: neighbours in the middle of the key space (one or two key ranges hold them all, which is what makes the
    batch too skewed for the plain range path), the last two at the ends of the key space"""
    h = cap // 3 + np.arange(k, dtype=np.int64)
    h[-1], h[-2] = cap - 1, 0
    return h.astype(np.uint32)


def _mix(rng, cap, n, head, counts, tail_from=None):
    """counts[i] requests of head[i] and a uniform tail, in random order"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() <= n
    m = n - int(counts.sum())
    tail = rng.integers(0, cap, m) if tail_from is None else tail_from[rng.integers(0, len(tail_from), m)]
    return rng.permutation(np.concatenate([np.repeat(head, counts), tail.astype(np.uint32)])).astype(np.uint32)


def _runs_of(slots, ref, head):
    """(A, length, first and last allowed request in different tiles) of every head slot's run in this batch -- from the
    oracle's decisions alone"""
    order = np.argsort(slots, kind="stable")
    ss = slots[order]
    out = []
    for a, b in zip(np.searchsorted(ss, head, "left"), np.searchsorted(ss, head, "right")):
        if a == b or ref.status[order[a]] != 0:
            continue
        idx = order[a:b]                           # the run's requests in queue order
        A = int(ref.allowed[idx].sum())
        assert ref.allowed[idx[:A]].all()          # one timestamp, one quantity: the allowed requests of a run are its first A
        out.append((A, int(b - a), bool(A >= 2 and idx[0] // TILE != idx[A - 1] // TILE)))
    return out


def _tally(runs):
    return {"partial": sum(1 < A < L for A, L, _ in runs), "cross": sum(c for _, _, c in runs),
            "a0": sum(A == 0 for A, _, _ in runs), "a1": sum(A == 1 for A, _, _ in runs), "full": sum(A == L for A, L, _ in runs)}


class _Run:
    """One engine and one oracle fed the same batches: every batch's decision bytes at once, the resident state of every slot
    touched on request (every case asks once in the middle of its stream), and again at the end with the counters, the self
    check and which batches took the form.  Used as a context manager: the engine is closed whatever happens."""

    def __init__(self, mp, cap, max_n, fixed, plan=None, tiers=None, env=None):
        import throttlecrab_amd as t
        mp.setenv("TCGPU_HOT_THREAD", "0")
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        self.t, self.cap = t, cap
        self.eng = t.Engine(cap, max_n, fixed_params=fixed)
        try:
            self.eng.use_torch_stream()
            self.orc = _oracle(cap)
            self.plan = plan
            if plan is not None:
                self.eng.register_params_uniform(*plan)
            else:
                # tiers = (slots, burst, count, period): registered slot by slot; every other slot stays unregistered (InvalidRateLimit)
                slots, b, c, p = tiers
                self.eng.register_params(b, c, p, slots=slots)
                self.B, self.C, self.P = (np.zeros(cap, np.int64) for _ in range(3))
                self.B[slots], self.C[slots], self.P[slots] = b, c, p
        except Exception:
            self.eng.close()
            raise
        self.now, self.paths, self.runs, self.touched = T0, [], [], []
        self.sums = np.zeros(3, np.int64)          # allowed, denied, errors -- the oracle's
        self.majority = []

    def step(self, slots, dt_ns, q=1, head=None, out=None):
        self.now += dt_ns
        if self.plan is not None:
            ref = self.orc.batch_slots(slots, *self.plan, q, self.now)
        else:
            ref = self.orc.batch_slots(slots, self.B[slots], self.C[slots], self.P[slots], q, self.now)
        d = _dev(slots.astype(np.int32))
        res = self.eng.rate_limit_batch_slots(d, registered=True, quantity=q, now_ns=self.now, want=("allowed",), inputs_ready=True,
                                              out=out, outputs_idle=out is not None)
        path = self.eng.info()["grouping_path"]
        _sync()    # the notes and hints this batch published are there when the next call looks
        i = len(self.paths)
        bad = np.nonzero(_host(res.allowed)[:len(slots)] != ref.allowed)[0]
        assert bad.size == 0, (f"batch {i} ({path}, n={len(slots)}): {bad.size} decisions differ, first at {bad[:6]} slots {slots[bad[:6]]} "
                               f"want {ref.allowed[bad[:6]]}")
        self.paths.append(path)
        self.touched.append(np.unique(slots))
        ok = ref.status == 0
        self.sums += (int(ref.allowed.sum()), int((ok & (ref.allowed == 0)).sum()), int((~ok).sum()))
        self.majority.append(float(ref.allowed.mean()))
        if head is not None and path == HOT:
            self.runs += _runs_of(slots, ref, head)
        return ref

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()    # (a failed comparison must not leave the engine, and its device memory, to the garbage collector)
        return False

    def check_state(self):
        assert_state_same(self.eng, self.orc, np.unique(np.concatenate(self.touched)))

    def finish(self, phases=(0,)):
        """phases: the batches at which a phase of the stream starts -- only a phase's first four batches may miss the form"""
        self.check_state()
        c = self.eng.counters()
        assert (c["allowed"], c["denied"], c["errors"]) == tuple(int(v) for v in self.sums), (c, self.sums)
        assert self.eng.selfcheck() == 0
        info = self.eng.info()
        self.eng.close()
        n = len(self.paths)
        assert self.paths.count(HOT) * 3 >= 2 * n, self.paths
        for i, p in enumerate(self.paths):
            assert p == HOT or i - max(s for s in phases if s <= i) < 4, (i, self.paths)
        return info


# ---- cases 1 and 2: run once each, shared by their tests and by the test of what they cover together ----
N12, BATCHES12 = 20_000, 20
COUNTS1 = [4000, 2500, 1500, 1000, 800] + [120] * 35      # 40 hot slots, 14 000 of a batch's 20 000 requests
CASE1 = [(cap, fixed, q) for cap in (70_001, 1_000_003) for fixed in (True, False) for q in (1, 3)]
CASE2 = [(cap, fixed) for cap in (70_001, 1_000_003) for fixed in (True, False)]
_DONE = {}


def _case1(cap, fixed, q):
    """one plan with a large burst and a fast refill: the five long runs are drained and refilled by the time steps (partial
    allowances in the thousands, spread over all five tiles), the 35 short ones stay allowed"""
    with pytest.MonkeyPatch.context() as mp, _Run(mp, cap, N12, fixed, plan=FAST) as run:
        rng = np.random.default_rng(cap % 1000 + 2 * fixed + q)
        head = _head(cap, len(COUNTS1))
        for b in range(BATCHES12):
            run.step(_mix(rng, cap, N12, head, COUNTS1), STEPS_NS[(b - 1) % 5] if b else 0, q=q, head=head)
            if b == BATCHES12 // 2:
                run.check_state()
        info = run.finish()
        assert info["hot_slots"] == len(head), info
        return _tally(run.runs)


# 41 hot slots (every run at least the 32 requests that are noted), 15 215 of 20 000 requests; the last one: unregistered
COUNTS2 = [3000, 2000, 1500, 1000, 900, 800, 700, 600, 400, 300, 200, 100] + [64, 48, 40, 33] * 7 + [2420]


def _case2(cap, fixed):
    """plans by slot, four tiers, hot slots in every one of them, one hot slot without a plan: its requests are errors (the hot
    role's HOT_ERR: byte 0, counted as errors, cell untouched)"""
    rng = np.random.default_rng(cap % 1000 + 2 * fixed)
    head = cap // 3 + np.arange(len(COUNTS2), dtype=np.int64)
    head[-2], head[-3] = cap - 1, 0
    head = head.astype(np.uint32)
    orphan = int(head[-1])
    reg = np.setdiff1d(np.arange(cap, dtype=np.uint32), [orphan])
    tier = np.array(TIERS, dtype=np.int64)[reg % 4]
    with pytest.MonkeyPatch.context() as mp, \
            _Run(mp, cap, N12, fixed, tiers=(reg, tier[:, 0].copy(), tier[:, 1].copy(), tier[:, 2].copy())) as run:
        for b in range(BATCHES12):
            ref = run.step(_mix(rng, cap, N12, head, COUNTS2), STEPS_NS[(b - 1) % 5] if b else 0, head=head)
            assert int((ref.status != 0).sum()) >= COUNTS2[-1]
            if b == BATCHES12 // 2:
                run.check_state()
        info = run.finish()
        assert run.orc.peek(orphan)[2] is False and info["hot_slots"] == len(head), info
        return _tally(run.runs)


def _once(key):
    if key not in _DONE:
        try:
            _DONE[key] = (_case1 if len(key) == 3 else _case2)(*key)
        except Exception as e:
            # (a stream that failed is not run a second time for the coverage test: what it said is kept -- the text, not the
            # exception with its frames -- and said again)
            _DONE[key] = f"the stream {key} failed: {type(e).__name__}: {e}"
            raise
    if isinstance(_DONE[key], str):
        raise AssertionError(_DONE[key])
    return _DONE[key]


@pytest.mark.parametrize("cap,fixed,q", CASE1)
def test_partial_allowance_across_tiles(cap, fixed, q):
    t = _once((cap, fixed, q))
    # (this stream alone, from the oracle: runs that are cut somewhere inside, in another tile than they start in, and drained ones)
    assert t["partial"] >= 10 and t["cross"] >= 10 and t["a0"] >= 1 and t["full"] >= 1, t


@pytest.mark.parametrize("cap,fixed", CASE2)
def test_per_slot_plans_and_an_unregistered_hot_slot(cap, fixed):
    t = _once((cap, fixed))
    assert t["partial"] >= 10 and t["a1"] >= 1, t


def test_cases_1_and_2_cover_the_rank_arithmetic():
    """what the rank form had to work out in the batches it was reported for, counted from the oracle's decisions"""
    tot = {}
    for key in CASE1 + CASE2:
        for k, v in _once(key).items():
            tot[k] = tot.get(k, 0) + int(v)
    assert tot["partial"] >= 10 and tot["cross"] >= 10, tot
    assert tot["a0"] >= 1 and tot["a1"] >= 1 and tot["full"] >= 1, tot


@pytest.fixture
def open_run(monkeypatch):
    """_Run(...) for a test that holds it for its whole body: closed when the test ends, however it ends"""
    made = []

    def make(*args, **kw):
        made.append(_Run(monkeypatch, *args, **kw))
        return made[-1]
    yield make
    for r in made:
        r.eng.close()


# ---- case 3 ----
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "wide"])
def test_vacant_and_expired_hot_cells_under_an_installed_list(fixed, open_run):
    """between two batches of the form: a pause longer than the tolerance (every hot cell expired, still resident), a sweep (vacant),
    and -- wide layout -- values planted through the store calls: i64::MAX, a timestamp long past, a ttl of 0"""
    cap, n = 70_001, 20_000
    rng = np.random.default_rng(3 + fixed)
    run = open_run(cap, n, fixed, plan=FAST)
    head = _head(cap, len(COUNTS1))

    def batches(k, first_dt):
        for j in range(k):
            run.step(_mix(rng, cap, n, head, COUNTS1), first_dt if j == 0 else STEPS_NS[j % 5], head=head)

    batches(6, 0)
    batches(2, 10 * 10**9)                                   # expired, not swept
    run.check_state()
    run.now += 10 * 10**9
    assert run.eng.sweep_expired(run.now) == run.orc.sweep(run.now) > len(head)
    batches(2, 1_000_000)                                    # vacant
    if not fixed:
        key = lambda s: int(s).to_bytes(4, "little")
        run.now += 10 * 10**9                                # (every cell expired again: set_if_not_exists takes them)
        for who in (run.eng, run.orc):
            assert who.set_if_not_exists_with_ttl(key(head[0]), 2**63 - 1, 10**9, run.now) is True
            assert who.set_if_not_exists_with_ttl(key(head[1]), T0 - 10 * 10**9, 10**9, run.now) is True
            assert who.set_if_not_exists_with_ttl(key(head[2]), run.now + 1000, 0, run.now) is True
            assert who.set_if_not_exists_with_ttl(key(head[3]), run.now, 10**9, run.now) is True
            assert who.compare_and_swap_with_ttl(key(head[3]), run.now, 2**63 - 1, 10**9, run.now) is True
        batches(2, 1000)
        run.now += 1000
        for who in (run.eng, run.orc):                       # the same into live cells that the form has just written
            old = who.get(key(head[4]), run.now)
            assert old is not None and who.compare_and_swap_with_ttl(key(head[4]), old, T0 - 10 * 10**9, 10**9, run.now) is True
            old = who.get(key(head[5]), run.now)
            assert old is not None and who.compare_and_swap_with_ttl(key(head[5]), old, old, 0, run.now) is True
        batches(2, 1000)
    run.finish()
    assert run.paths.count(HOT) == len(run.paths) - 1, run.paths


# ---- case 4 ----
@pytest.mark.parametrize("majority", ["allowed", "denied"])
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "wide"])
def test_preset_decision_bytes_pass_through_the_hot_role(fixed, majority, open_run):
    """TC_B_OUTPUTS_IDLE with a ring of three result arrays: the partition presets the bytes to the majority decision of a recent
    batch, the hot role stores the other one only -- a stream for either polarity, and the bytes behind the batch stay as they were"""
    import throttlecrab_amd as t
    cap, nb = 70_001, 16
    rng = np.random.default_rng(4 + fixed)
    if majority == "denied":
        # six runs of 4 500 that regain 300, 0, 600, 120, 300 tokens: at most (6 * 600 + 5 768) / 32 768 = 29 % of a batch allowed
        n, counts, steps = 32_768, [4500] * 6, (5_000_000, 0, 10_000_000, 2_000_000, 5_000_000)
    else:
        # three runs that are cut or denied whole (3 000, 300, 0, 1 200, 0 tokens), 27 of 400 that never are: at least 10 800 + 2 700
        # of 20 000 allowed
        n, counts, steps = 20_000, [2500, 2200, 1800] + [400] * 27, STEPS_NS
    run = open_run(cap, n, fixed, plan=FAST)
    head = _head(cap, len(counts))
    ring = [_dev(np.zeros(n + 64, np.uint8)) for _ in range(3)]
    for b in range(nb):
        m = n - (b % 4) * 33                                 # (ragged: an array of the ring serves batches of several sizes)
        ring[b % 3].fill_(7)
        _sync()
        run.step(_mix(rng, cap, m, head, [c - b % 4 for c in counts]), steps[(b - 1) % 5] if b else 0, head=head,
                 out=t.BatchResult(allowed=ring[b % 3][:m]))
        assert (_host(ring[b % 3])[m:] == 7).all(), f"batch {b}: bytes behind the batch were written"
        if b == nb // 2:
            run.check_state()
    run.finish()
    # the oracle's share of allowed requests, batch by batch: the fill value (a recent batch's majority) is this stream's from the
    # second batch on -- and the hot role has plenty of the OTHER decision to store: runs cut inside
    frac = run.majority[1:]
    assert all(f > 0.6 for f in frac) if majority == "allowed" else all(f < 0.4 for f in frac), frac
    # (batches 4 .. 15 are the form's: ten of their time steps leave a run of the first stream cut inside, five one of the second)
    part = _tally(run.runs)["partial"]
    assert part >= (6 * 10 if majority == "denied" else 3 * 5), part


# ---- case 5 ----
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "wide"])
def test_more_hot_candidates_than_the_list_holds(fixed, open_run):
    """600 slots with runs of at least TCGPU_HOT_MIN = 8 requests: the 512 longest make the list, the other 88 are grouped by the
    ranges and evaluated by the sorted part -- exact either way"""
    cap, n, nb = 70_001, 40_000, 12
    rng = np.random.default_rng(5 + fixed)
    plan = (30, 6000, 1)                                     # ei = 166 us, dvt ~ 4.8 ms: at most 30 of a run are allowed
    run = open_run(cap, n, fixed, plan=plan, env={"TCGPU_HOT_MIN": "8"})
    head = (cap // 2 + np.arange(600)).astype(np.uint32)
    counts = 12 + (np.arange(600) * 98) // 599               # 12 .. 110, 36 550 requests in all; the 88 shortest: 12 .. 26
    sizes = []
    for b in range(nb):
        run.step(_mix(rng, cap, n, head, counts), STEPS_NS[(b - 1) % 5] if b else 0, head=head)
        sizes.append(run.eng.info()["hot_slots"])
        if b == nb // 2:
            run.check_state()   # (the 88 slots below the cut are in it too: their cells come from the sorted part)
    run.finish()
    assert sizes[1:] == [512] * (nb - 1), sizes
    assert _tally(run.runs)["partial"] >= 100


# ---- case 6 ----
RAGGED = [20_480, 16_384, 16_385, 18_431, 18_432, 18_433, 20_479, 20_480, 20_481, 16_383, 16_384, 18_433, 20_481, 18_431, 16_385]


@pytest.mark.parametrize("cap", [70_001, 1_000_003])
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "wide"])
def test_ragged_sizes_inside_one_stream(fixed, cap, open_run):
    """tile, half-tile and smallest-size edges of the form (a hot-role block per half tile of 2 048 requests), and a batch one
    request below the form between two batches of it"""
    rng = np.random.default_rng(6 + fixed + cap % 7)
    run = open_run(cap, max(RAGGED), fixed, plan=FAST)
    head = _head(cap, 40)
    for b, n in enumerate(RAGGED):
        counts = [n // 5, n // 8, n // 10] + [n // 100] * 37     # ~ 79 % of the batch
        slots = _mix(rng, cap, n, head, counts)
        slots[-1], slots[0] = head[0], head[1]                   # (a hot request in the last, ragged, place)
        run.step(slots, STEPS_NS[(b - 1) % 5] if b else 0, head=head)
        if n == 16_383 or b == 4:
            run.check_state()   # (in the middle of the first phase, and what the batch that left the form took over and left behind)
    below = RAGGED.index(16_383)
    run.finish(phases=(0, below))
    assert [i for i, p in enumerate(run.paths) if p != HOT] == [0, below], run.paths


# ---- case 7 ----
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "wide"])
def test_the_sorted_part_in_more_than_one_stretch(fixed, open_run):
    """k_eval_lean_hot's loop over stretches (bid += cold_grid).  TCGPU_EVAL_ITEMS=1: a block of the sorted part takes 256
    positions.  The host sizes that part's grid from a recent batch's cold count scaled to this batch: 1.25 * est / 256 + 32
    blocks.  The stream's hot slots take 70 % of each batch of 20 000, so est = 6 000 and the grid is 7 500 / 256 + 32 = 61
    blocks; the last batch holds no hot request at all: its sorted part is 20 000 positions = 79 stretches, so 18 blocks
    take a second one.  61 + 10 hot-role blocks are co-resident many times over (nothing here waits for a block that is not).
    The test cannot SEE that a second stretch ran: it rests on this arithmetic (slots.hip, launch_eval_items: the cold hint is the
    previous batch's count because every batch here is followed by a synchronisation) -- whoever changes how that grid is sized,
    the slack of 32 blocks included, must redo it here."""
    cap, n = 70_001, 20_000
    rng = np.random.default_rng(7 + fixed)
    run = open_run(cap, n, fixed, plan=FAST, env={"TCGPU_EVAL_ITEMS": "1"})
    counts = [3000, 2000, 1000] + [216] * 37                 # 13 992 of 20 000
    head = _head(cap, len(counts))
    cold = np.setdiff1d(np.arange(cap, dtype=np.uint32), head)
    for b in range(8):
        run.step(_mix(rng, cap, n, head, counts, tail_from=cold), STEPS_NS[(b - 1) % 5] if b else 0, head=head)
    run.check_state()
    run.step(_mix(rng, cap, n, head, [0] * len(counts), tail_from=cold), 5_000_000)
    run.check_state()   # (every cell here was stored by the sorted part's stretches; the hot cells must be as they were)
    assert run.paths[-1] == HOT, run.paths
    # ... and the other way round: a grid sized by a batch without hot requests (the whole batch's) for the usual sorted part
    run.step(_mix(rng, cap, n, head, counts, tail_from=cold), 5_000_000, head=head)
    run.step(_mix(rng, cap, n, head, counts, tail_from=cold), 0, head=head)
    run.finish()
    assert run.paths[1:] == [HOT] * 10, run.paths
