"""tc_export_live / tc_import_live: the live entries of an engine as an arena (against the engine's own host introspection), and
merged into another engine (decisions against the CPU oracle, cells against the merge rule in plain Python).  Integer-exact."""
import ctypes as C

import numpy as np
import pytest

from tests import kat

pytestmark = pytest.mark.gpu

LENS = (0, 1, 15, 16, 17, 112, 113, 300)  # both sides of the Entry and KeyRec inline limits, and the overflow arena
FIELDS = ("allowed", "limit", "remaining", "reset_after_ns", "retry_after_ns", "status")
CAP, SENT, S = 5000, 0x5A5A5A5A, 10**9
PLANS = np.array([[5, 10, 60], [2, 100, 10], [50, 10, 60]])  # entries stay for ~30 s, ~0.2 s, ~300 s


def _keys(n, first=0):
    rng = np.random.default_rng(5)
    pad = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    return list(dict.fromkeys((b"%d:" % i + pad)[:LENS[i % len(LENS)]] for i in range(first, first + n)))


def _run(eng, orc, keys, ids, now, mode):
    """one batch with per-request plans on the engine and on the model -> (engine's results, model's)"""
    from oracle import oracle as O
    b, c, p = (np.ascontiguousarray(PLANS[np.asarray(ids) % 3, k]) for k in range(3))
    if mode == "keys":
        kb, ko = O.pack_keys([keys[i] for i in ids])
        return (eng.rate_limit_batch_keys(kb, ko, max_burst=b, count_per_period=c, period=p, quantity=1, now_ns=now),
                None if orc is None else orc.batch_keys(kb, ko, b, c, p, 1, now))
    sl = np.asarray(ids, np.uint32)
    return (eng.rate_limit_batch_slots(sl, max_burst=b, count_per_period=c, period=p, quantity=1, now_ns=now),
            None if orc is None else orc.batch_slots(sl, b, c, p, 1, now))


def _history(mode, with_model=False):
    """an engine of CAP slots after two batches and a sweep between them: at t0 + 20 s some entries are live, some expired but
    still resident, and the sweep's free slots lie between them"""
    import throttlecrab_amd as t
    from oracle import oracle as O
    t0 = kat.load()["t0_ns"]
    eng = t.Engine(CAP, 4096, key_mode=mode == "keys")
    keys = _keys(3000) if mode == "keys" else None
    orc = None if not with_model else (O.AdaptiveOracle(capacity=100000, created_ns=t0, auto_cleanup=False) if mode == "keys" else O.DenseOracle(CAP))
    ids = np.arange(len(keys)) if mode == "keys" else np.random.default_rng(2).permutation(CAP)[:3000]
    _run(eng, orc, keys, ids[:1500], t0, mode)
    eng.sweep_expired(t0 + S)
    _run(eng, orc, keys, ids[1500:], t0 + S, mode)
    return eng, keys, orc, t0


@pytest.fixture(scope="module")
def engines():
    out = {m: _history(m) for m in ("keys", "slots")}
    yield out
    for eng, *_ in out.values():
        eng.close()


def _slot_keys(eng, slots):
    sl, off, buf = np.ascontiguousarray(slots, np.uint32), np.zeros(len(slots) + 1, np.uint32), np.zeros(300 * len(slots) + 1, np.uint8)
    eng._check(eng._lib.tc_slot_keys(eng._h, len(sl), sl.ctypes.data, buf.ctypes.data, buf.size, off.ctypes.data))
    return buf[:off[-1]], off


def _expected(eng, mode, now, first, n, world, only):
    """read_state (+ slot_keys, route_keys) -> slot, tat, expiry, key_off, key_bytes of the page's live entries, ascending"""
    from throttlecrab_amd import sharded
    tat, exp = eng.read_state(first, n)
    slots = np.nonzero(exp > np.uint64(now))[0] + first
    kb, ko = _slot_keys(eng, slots) if mode == "keys" else (np.zeros(0, np.uint8), np.zeros(len(slots) + 1, np.uint32))
    if world >= 2:
        keep = np.nonzero(sharded.route_keys(np.append(kb, np.uint8(0)), ko, world) == only)[0]
        kb = np.concatenate([kb[ko[i]:ko[i + 1]] for i in keep] + [np.zeros(0, np.uint8)])
        ko, slots = np.concatenate([[0], np.cumsum(ko[keep + 1] - ko[keep])]), slots[keep]
    return slots, tat[slots - first], exp[slots - first], ko.astype(np.int64), kb


def _outputs(eng, cap_e, cap_b):
    """sentinel-filled outputs with slack behind the room the call is told of"""
    import torch
    o = {k: torch.full((cap_e + 8,), SENT, dtype=dt, device="cuda") for k, dt in (("slot", torch.int32), ("tat", torch.int64), ("expiry", torch.int64))}
    o.update(count=torch.full((2,), SENT, dtype=torch.int64, device="cuda"), cap_entries=cap_e, cap_bytes=cap_b)
    if eng.key_mode:
        o.update(key_off=torch.full((cap_e + 9,), SENT, dtype=torch.int32, device="cuda"), key_bytes=torch.full((cap_b + 64,), SENT & 0xFF, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return o


def _untouched(o, entries=0, nbytes=0, off_words=0):
    return (all((o[k][entries:] == SENT).all() for k in ("slot", "tat", "expiry")) and
            ("key_off" not in o or ((o["key_off"][off_words:] == SENT).all() and (o["key_bytes"][nbytes:] == SENT & 0xFF).all())))


@pytest.mark.parametrize("mode,world,only", [("keys", 0, 0), ("keys", 3, 1), ("slots", 0, 0)])
@pytest.mark.parametrize("first,n", [(0, CAP), (700, 2900), (2047, 1)])  # whole capacity; starts and ends inside a tile; one slot
def test_export_equals_introspection(engines, mode, world, only, first, n):
    eng, _, _, t0 = engines[mode]
    now = t0 + 20 * S
    slots, tat, exp, ko, kb = _expected(eng, mode, now, first, n, world, only)
    if (first, n) == (0, CAP):  # live entries and expired residents; key mode: the first tile's bytes do not fit the kernel's 48 KiB stage
        assert 100 < len(slots) < int((eng.read_state(0, CAP)[1] > 0).sum()) and (mode == "slots" or world or ko[np.searchsorted(slots, 2048)] > 48 * 1024)
    host, before = eng.host_alloc(3, np.uint64), eng.counters()
    o = eng.export_live(_outputs(eng, CAP, 200_000), now, first, n, world, only, host_counts=host, tag=7 + first)
    eng.synchronize()
    k = len(slots)
    assert o["count"].tolist() == [k, len(kb)] and host.tolist() == [k, len(kb), 7 + first]
    assert np.array_equal(o["slot"][:k].cpu().numpy(), slots) and np.array_equal(o["tat"][:k].cpu().numpy(), tat)
    assert np.array_equal(o["expiry"][:k].cpu().numpy().view(np.uint64), exp)
    if mode == "keys":
        assert np.array_equal(o["key_off"][:k + 1].cpu().numpy(), ko) and np.array_equal(o["key_bytes"][:len(kb)].cpu().numpy(), kb)
        assert eng.debug_check_keys() == 0
    assert _untouched(o, k, len(kb), k + 1) and eng.selfcheck() == 0 and eng.counters() == before


@pytest.mark.parametrize("mode", ["keys", "slots"])
def test_overflow_writes_counts_only(engines, mode):
    eng, _, _, t0 = engines[mode]
    slots, _, _, ko, kb = _expected(eng, mode, t0 + 20 * S, 0, CAP, 0, 0)
    for cap_e, cap_b in [(len(slots) - 1, 200_000)] + ([(CAP, len(kb) - 1)] if mode == "keys" else []):
        o = eng.export_live(_outputs(eng, cap_e, cap_b), t0 + 20 * S)
        eng.synchronize()
        assert o["count"].tolist() == [len(slots), len(kb)] and _untouched(o)


@pytest.mark.parametrize("mode", ["keys", "slots"])
def test_round_trip_preserves_decisions(mode):
    import throttlecrab_amd as t
    a, keys, orc, t0 = _history(mode, with_model=True)
    b = t.Engine(8000, 4096, key_mode=mode == "keys")
    o = a.export_live(a.export_buffers(CAP, 200_000), t0 + 20 * S)
    a.synchronize()
    k = int(o["count"][0])
    for lo, hi in ((0, k // 2), (k // 2, k)):  # two imports; the second arena's offsets do not start at 0
        cnt = b.import_live(hi - lo, o["tat"][lo:hi], o["expiry"][lo:hi], slot=o["slot"][lo:hi], key_bytes=o.get("key_bytes"),
                            key_off=o["key_off"][lo:hi + 1] if mode == "keys" else None)
        b.synchronize()
        assert cnt.tolist() == [hi - lo, 0]
    # exported keys, expired ones, new ones, duplicates inside the batch
    keys = keys + _keys(400, 3000) if mode == "keys" else None
    ids = np.random.default_rng(9).integers(0, len(keys) if mode == "keys" else CAP, 3500)
    ra, ref = _run(a, orc, keys, ids, t0 + 21 * S, mode)
    rb, _ = _run(b, None, keys, ids, t0 + 21 * S, mode)
    for f in FIELDS:
        want = getattr(ref, f).astype(np.int64)
        assert np.array_equal(getattr(ra, f).astype(np.int64), want) and np.array_equal(getattr(rb, f).astype(np.int64), want), f
    assert len(set(ref.allowed)) == 2 and b.selfcheck() == 0 and (mode == "slots" or b.debug_check_keys() == 0)
    a.close(), b.close()


@pytest.mark.parametrize("mode", ["keys", "slots"])
def test_merge_rule(mode):
    import torch
    import throttlecrab_amd as t
    from oracle import oracle as O
    t0 = kat.load()["t0_ns"]
    eng = t.Engine(64, 64, key_mode=mode == "keys")
    names = [3, 9, 17, 20, 33] if mode == "slots" else [b"resident-a", b"b", b"c" * 113, b"", b"e" * 40]
    where = (lambda k: k) if mode == "slots" else eng.lookup_slot
    _run(eng, None, names, [0, 1] if mode == "keys" else names[:2], t0, mode)  # two residents
    res = {k: tuple(int(v[0]) for v in eng.read_state(where(k), 1)) for k in names[:2]}
    (ta, xa), (tb, xb) = res[names[0]], res[names[1]]
    # resident TAT below / above the imported one; negative TAT into a vacant cell; vacant entry; duplicates; slot out of range
    entries = [(names[0], ta + 1000, xa - 5), (names[1], tb - 1000, xb + 5), (names[2], -9, t0 + 7), (names[3], 1, 0), (names[4], -30, t0 + 3),
               (names[4], -20, t0 + 9)] + ([(64 + 5, 4, t0 + 1)] if mode == "slots" else [])
    good = [e for e in entries if e[2] != 0 and (mode == "keys" or e[0] < 64)]
    kb, ko = O.pack_keys([e[0] for e in entries]) if mode == "keys" else (None, None)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).cuda()
    cnt = eng.import_live(len(entries), dev([e[1] for e in entries], np.int64), dev([e[2] for e in entries], np.int64),
                          slot=dev([e[0] for e in entries], np.int32) if mode == "slots" else None,
                          key_bytes=dev(kb, np.uint8) if mode == "keys" else None, key_off=dev(ko.astype(np.int32), np.int32) if mode == "keys" else None)
    eng.synchronize()
    assert cnt.tolist() == [len(good), len(entries) - len(good)]
    for k in {e[0] for e in good}:
        rt, rx = res.get(k, (0, 0))
        want = (max([e[1] for e in good if e[0] == k] + ([rt] if rx else [])), max([rx] + [e[2] for e in good if e[0] == k]))
        assert tuple(int(v[0]) for v in eng.read_state(where(k), 1)) == want, k
    assert eng.selfcheck() == 0 and (mode == "slots" or eng.debug_check_keys() == 0)
    eng.close()


@pytest.mark.parametrize("bad", [dict(first_slot=CAP), dict(n_slots=CAP + 1), dict(flags=1), dict(world=65), dict(world=3, only=3), dict(out_tat=None), dict(n=4097)])
def test_refusals_change_nothing(engines, bad):
    import throttlecrab_amd as t
    from oracle import oracle as O
    from throttlecrab_amd import _lib as L
    eng, keys, _, t0 = engines["keys"]
    kb, ko = O.pack_keys(keys[:64])
    peek = lambda: eng.peek_batch_keys(kb, ko, max_burst=5, count_per_period=10, period=60, quantity=1, now_ns=t0 + 2 * S).throttle.copy()
    before, o = peek(), _outputs(eng, CAP, 200_000)
    if "n" in bad:
        with pytest.raises(t.TcError) as ei:
            eng.import_live(bad["n"], o["tat"], o["expiry"], key_bytes=o["key_bytes"], key_off=o["key_off"])
    else:
        x = L.tc_export(struct_size=C.sizeof(L.tc_export), n_slots=CAP, **{k: eng._ptr(o.get(k[4:])) for k in ("out_tat", "out_expiry", "out_count", "out_key_bytes", "out_key_off")})
        for k, v in bad.items():
            setattr(x, k, v)
        with pytest.raises(t.TcError) as ei:
            eng._check(eng._lib.tc_export_live(eng._h, C.byref(x)))
    eng.synchronize()
    assert ei.value.code == L.TC_E_INVALID_ARG and np.array_equal(peek(), before) and _untouched(o) and (o["count"] == SENT).all()
    fixed = t.Engine(100, 100, fixed_params=True)
    for call in (lambda: fixed.export_live(o, t0), lambda: fixed.import_live(1, o["tat"], o["expiry"], slot=o["slot"])):
        with pytest.raises(t.TcError) as ei:
            call()
        assert ei.value.code == L.TC_E_UNSUPPORTED
    fixed.close()
