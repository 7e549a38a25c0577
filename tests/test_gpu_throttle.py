"""tc_throttle_batch_slots / _keys: batches answered as 16-byte tc_throttle records (ThrottleResponse without `limit`, whole
seconds, 34 bits per value), compared record by record with the oracle on every path a batch can take; the resident state and
the kernels' self-check once per case."""
import ctypes as C

import numpy as np
import pytest

import throttlecrab_amd as t
from oracle import oracle as O
from tests import kat
from throttlecrab_amd import _lib as L
from throttlecrab_amd import workload as W

pytestmark = pytest.mark.gpu
T0 = kat.load()["t0_ns"]
S = 10**9
FIELDS = ("allowed", "limit", "remaining", "reset_after_ns", "retry_after_ns", "status")
PLANS = np.array([(5, 10, 60), (100, 1000, 3600), (40, 7, 3), (2, 2, 2), (1, 10, 1), (0, 10, 60)], dtype=np.int64)   # (the last: an invalid triple)


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    monkeypatch.setenv("TCGPU_HOST_CHUNK", "65536")


def _stream(rng, n, n_keys, rnd):
    ids = rng.integers(0, n_keys, n)
    pl = PLANS[(ids * 7 + rnd) % len(PLANS)]
    q = rng.integers(0, 3, n).astype(np.int64)
    now = (T0 + rnd * S + np.sort(rng.integers(0, S, n))).astype(np.int64)
    return ids, pl, q, now


def _check(thr, ref, ctx, order=None):
    """every record against the oracle: the three values, and the whole `bits` word (allowed, status, TC_T_WIDE, high bits, spare bits)"""
    pick = (lambda a: a[order]) if order is not None else (lambda a: a)
    ok = pick(ref.status) == 0
    exp = {k: np.where(ok, pick(v).astype(np.int64), 0) for k, v in (("remaining", ref.remaining), ("reset_after_s", ref.reset_after_ns // S),
                                                                       ("retry_after_s", ref.retry_after_ns // S))}
    bits = (pick(ref.allowed).astype(np.int64) & ok) | (pick(ref.status).astype(np.int64) << 1)
    for k, name in enumerate(exp):
        bits |= (exp[name] >= 1 << 34).astype(np.int64) << 3
        exp[name] = np.minimum(exp[name], (1 << 34) - 1)
        bits |= (exp[name] >> 32) << (8 + 2 * k)
    got = t.Engine.unpack_throttle(thr)
    for name, want in dict(exp, bits=bits).items():
        bad = np.nonzero(got[name] != want)[0]
        assert bad.size == 0, f"{ctx}: {name} differs at {bad[:8]}: got {got[name][bad[:8]]} want {want[bad[:8]]}"


def _state_same(eng, orc):
    tat, exp = eng.read_state(0, eng.capacity)
    otat, oexp, occ = orc.dump()
    assert np.array_equal(exp[~occ], np.zeros((~occ).sum(), np.uint64)), "a slot the oracle never wrote is occupied"
    assert np.array_equal(tat[occ], otat[occ]) and np.array_equal(exp[occ], oexp[occ]), "resident state differs"
    assert eng.selfcheck() == 0


def _pinned(eng, a):
    h = eng.host_alloc(a.size, a.dtype)
    h[:] = a.reshape(-1)
    return h


def _pinned_out(eng, n):
    return t.BatchResult(throttle=eng.host_alloc(4 * n, np.uint32).reshape(n, 4))


@pytest.mark.parametrize("n", [700, 5000, 200_001])
@pytest.mark.parametrize("mode", ["pageable", "pinned", "async_ring", "device"])
def test_slot_batches(n, mode):
    """per-request plans, quantities 0-2, sorted per-request timestamps, duplicates: the general kernel (and k_small_batch)"""
    import torch
    cap = 30_000
    eng, orc = t.Engine(cap, 1 << 18), O.DenseOracle(cap)
    eng.check_on_close = True
    rng = np.random.default_rng(n)
    held = []
    for rnd in range(4):
        ids, pl, q, now = _stream(rng, n, cap, rnd)
        slots = ids.astype(np.uint32)
        ref = orc.batch_slots(slots, pl[:, 0], pl[:, 1], pl[:, 2], q, now, threads=O.host_threads())
        cols = dict(max_burst=pl[:, 0].copy(), count_per_period=pl[:, 1].copy(), period=pl[:, 2].copy(), quantity=q, now_ns=now)
        if mode == "device":
            res = eng.rate_limit_batch_slots(torch.from_numpy(slots.astype(np.int32)).cuda(), want=("throttle",),
                                             **{k: torch.from_numpy(v).cuda() for k, v in cols.items()})
            torch.cuda.synchronize()
            _check(res.throttle, ref, f"round {rnd}")
        elif mode == "pageable":   # (the other outputs beside the records: written as before)
            res = eng.rate_limit_batch_slots(slots, want=FIELDS + ("throttle",), **cols)
            _check(res.throttle, ref, f"round {rnd}")
            for f in FIELDS:
                assert np.array_equal(getattr(res, f).astype(np.int64), getattr(ref, f).astype(np.int64)), f"round {rnd}: {f}"
        else:
            args = dict(want=("throttle",), out=_pinned_out(eng, n), **{k: _pinned(eng, v) for k, v in cols.items()})
            if mode == "pinned":
                _check(eng.rate_limit_batch_slots(_pinned(eng, slots), **args).throttle, ref, f"round {rnd}")
            else:
                held.append((eng.rate_limit_batch_slots(_pinned(eng, slots), async_=True, **args), ref, args))
    if held:
        eng.wait_batches()
        for i, (res, ref, _) in enumerate(held):
            _check(res.throttle, ref, f"async batch {i}")
    _state_same(eng, orc)
    eng.close()


@pytest.mark.parametrize("fixed,form,n,keys", [(False, "request_order", 5000, 300), (False, "grouped", 5000, 300), (True, "request_order", 5000, 300),
                                               (True, "grouped", 5000, 300), (False, "unique", 5000, 0), (False, "bucket", 20_000, 30_000)])
def test_registered_plans_one_timestamp_per_batch(fixed, form, n, keys):
    """uniform batches: k_eval_sorted's run form on duplicate-heavy keys (direct stores; quantity 0 in the last round: the parked
    stores and the commit launch), grouped rows (row k answers request order[k]), unique slots, and from 16 384 evenly spread
    requests the bucket path"""
    cap = 30_000
    eng, orc = t.Engine(cap, 1 << 16, fixed_params=fixed), O.DenseOracle(cap)
    eng.check_on_close = True
    rng = np.random.default_rng(11)
    pl = PLANS[rng.integers(0, 4, cap)]            # (burst >= 2: what the 8-byte layout registers)
    eng.register_params(pl[:, 0].copy(), pl[:, 1].copy(), pl[:, 2].copy())
    for rnd in range(3):
        slots = (rng.permutation(cap)[:n] if form == "unique" else rng.integers(0, keys, n)).astype(np.uint32)
        now = T0 + rnd * 400_000_000
        q = (1, 1, 0)[rnd]
        ref = orc.batch_slots(slots, pl[slots, 0], pl[slots, 1], pl[slots, 2], q, now)
        res = eng.rate_limit_batch_slots(slots, registered=True, quantity=q, now_ns=now, want=("throttle",), grouped=form == "grouped",
                                         unique=form == "unique")
        order = None
        if form == "grouped":
            order = res.order.astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(n))
        _check(res.throttle, ref, f"round {rnd}", order)
        assert form != "bucket" or q == 0 or eng.info()["grouping_path"] == "bucket path"
    _state_same(eng, orc)
    eng.close()


@pytest.mark.parametrize("n", [900, 150_000])
@pytest.mark.parametrize("mode", ["pageable", "pinned"])
def test_key_batches(n, mode):
    eng = t.Engine(60_000, 1 << 18, key_mode=True)
    eng.check_on_close = True
    orc = O.AdaptiveOracle(capacity=60_000, created_ns=T0, auto_cleanup=False)
    rng = np.random.default_rng(n + 1)
    for rnd in range(3):
        ids, pl, q, now = _stream(rng, n, 20_000, rnd)
        kb, ko = W.string_keys(ids, prefix=b"user:")
        ref = orc.batch_keys(kb, ko, pl[:, 0], pl[:, 1], pl[:, 2], q, now)
        cols = dict(max_burst=pl[:, 0].copy(), count_per_period=pl[:, 1].copy(), period=pl[:, 2].copy(), quantity=q, now_ns=now)
        if mode == "pageable":
            res = eng.rate_limit_batch_keys(kb, ko, want=("throttle",), **cols)
        else:
            res = eng.rate_limit_batch_keys(_pinned(eng, kb), _pinned(eng, ko), want=("throttle",), out=_pinned_out(eng, n),
                                            **{k: _pinned(eng, v) for k, v in cols.items()})
        _check(res.throttle, ref, f"round {rnd}")
    assert eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    eng.close()


def test_rejected_key_requests_are_answered_after_the_retry():
    """a table too small for its keys: the synchronous call sweeps and applies the rejected requests again -- their records
    are scattered back into the caller's array"""
    eng = t.Engine(4096, 1 << 14, key_mode=True)
    eng.set_sweep_policy("adaptive", created_ns=T0)
    orc = O.AdaptiveOracle(capacity=1 << 20, created_ns=T0, auto_cleanup=False)

    def run(first, now):
        kb, ko = W.string_keys(np.arange(first, first + len(now)), prefix=b"r:")
        res = eng.rate_limit_batch_keys(kb, ko, max_burst=2, count_per_period=10, period=1, quantity=1, now_ns=now, want=("throttle",))
        _check(res.throttle, orc.batch_keys(kb, ko, 2, 10, 1, 1, now), f"keys from {first}")

    run(0, np.full(3000, T0 + S, np.int64))          # entries live 0.2 s
    # 2 000 new keys into 1 096 free slots.  The call's first timestamp, which the sweep in front of it goes by, is 0.05 s later:
    # nothing has expired.  Its newest one, which the retry sweeps at, is 0.5 s later: everything has.
    now = np.full(2000, T0 + S + 5 * 10**8, np.int64)
    now[:10] = T0 + S + 5 * 10**7
    run(10_000, now)
    assert eng.sweep_stats()["retries"] == 1 and eng.counters()["errors"] == 0
    assert eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    eng.close()


def _edge_requests():
    """(slot, burst, count, period, quantity, now) rows.  Slot 1: ei = 10^9 ns exactly, timestamps 1 ns apart on both sides of
    whole seconds -- durations of k 10^9 - 1, k 10^9 and k 10^9 + 1 ns.  Slot 2: ei = 5 10^18 ns, reset_after beyond 2^32 s.
    Slot 3: burst 2^32 with quantity 0, remaining = 2^32.  Slots 4-6: negative quantity, invalid triple, now < 0."""
    b0 = (T0 // S + 1) * S
    rows = [(1, 5, 1, 1, 1, b0 + d) for d in (0, 1, 2)] + [(1, 5, 1, 1, 1, b0 + k * S + d) for k in range(1, 6) for d in (-1, 0, 1)]
    rows += [(2, 2, 1, 5 * S, 1, b0), (2, 2, 1, 5 * S, 1, b0 + 1), (2, 2, 1, 5 * S, 0, b0 + 2)]
    rows += [(3, 1 << 32, S, 1, 0, b0), (3, 1 << 32, S, 1, 1, b0 + 1)]
    rows += [(4, 5, 10, 60, -1, b0), (5, 0, 10, 60, 1, b0), (6, 5, 10, 60, 1, -5)]
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("n", [0, 5000], ids=["small_batch", "padded_to_5000"])
def test_edges_of_the_record(n):
    cap = 10_000
    edge = _edge_requests()
    rows = edge
    if n:   # the same requests, in the same order, among ordinary traffic on other slots
        rng = np.random.default_rng(5)
        ids, pl, q, now = _stream(rng, n - len(edge), cap - 100, 0)
        mine = np.zeros(n, bool)
        mine[rng.choice(n, len(edge), replace=False)] = True
        rows = np.empty((n, 6), np.int64)
        rows[mine], rows[~mine] = edge, np.column_stack([ids + 100, pl, q, now])
    eng, orc = t.Engine(cap, 1 << 16), O.DenseOracle(cap)
    eng.check_on_close = True
    cols = [np.ascontiguousarray(rows[:, k]) for k in range(6)]
    ref = orc.batch_slots(cols[0].astype(np.uint32), *cols[1:])
    ok = ref.status == 0
    # the cases are there (else this test would quietly stop covering bits 8-13 and the rounding)
    assert (ref.reset_after_ns[ok] // S >= 1 << 32).any() and (ref.remaining[ok] >= 1 << 32).any()
    assert {0, 1, S - 1} <= set((ref.reset_after_ns[ok] % S).tolist()) and sorted(set(ref.status.tolist())) == [0, 1, 2, 3]
    res = eng.rate_limit_batch_slots(cols[0].astype(np.uint32), max_burst=cols[1], count_per_period=cols[2], period=cols[3], quantity=cols[4],
                                     now_ns=cols[5], want=("throttle",))
    _check(res.throttle, ref, "edges")
    _state_same(eng, orc)
    eng.close()


@pytest.mark.parametrize("kind", ["slots", "keys"])
def test_a_null_or_misaligned_record_array_is_refused(kind):
    n = 2000
    eng = t.Engine(5000, 1 << 14, key_mode=kind == "keys")
    b, res, keep = eng._prepare(n, False, 5, 10, 60, 1, T0, False, False, ("throttle",), None)
    slots = np.arange(n, dtype=np.uint32)
    kb, ko = np.frombuffer(b"k" * n, np.uint8), np.arange(n + 1, dtype=np.uint32)
    b.slot, b.key_bytes, b.key_off = (slots.ctypes.data, None, None) if kind == "slots" else (None, kb.ctypes.data, ko.ctypes.data)
    call = getattr(eng._lib, "tc_throttle_batch_" + kind)
    for ptr in (None, res.throttle.ctypes.data + 4, res.throttle.ctypes.data + 8):
        assert call(eng._h, C.byref(b), ptr) == L.TC_E_INVALID_ARG
    assert eng.counters()["total"] == 0 and eng.counters()["keys_inserted"] == 0
    assert not eng.read_state(0, 5000)[1].any()
    assert call(eng._h, C.byref(b), res.throttle.ctypes.data) == 0 and eng.counters()["total"] == n
    eng.close()
