"""tc_peek_batch_keys / tc_peek_batch_slots: every answer equals the reference's rate_limit on a throw-away model that holds just
the key's live TAT (Python integers, no tolerance), and nothing in the engine changes."""
import ctypes as C

import numpy as np
import pytest
import torch

import throttlecrab_amd as t
from oracle import oracle as O
from oracle.pymodel import PyModel
from throttlecrab_amd import _lib as L

pytestmark = pytest.mark.gpu
T0 = 1_700_000_000 * 10**9
LENS = (0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 112, 113, 200)
PLANS = ((5, 10, 60), (3, 10, 1), (2, 100, 60), (0, 10, 60))  # the last one is invalid


def reference(get, keys, burst, count, period, q, now):
    """rows of (status, allowed, remaining, reset_after_ns, retry_after_ns): PyModel.rate_limit on {key: live tat} or {}"""
    rows = []
    for i, k in enumerate(keys):
        m, tat = PyModel(), get(k, int(now[i]))
        if tat is not None:
            m.data[k] = (tat, int(now[i]) + 1)
        st, al, _, rem, rs, rt = m.rate_limit(k, int(burst[i]), int(count[i]), int(period[i]), int(q[i]), int(now[i]))
        rows.append((st, int(al), rem, rs, rt))
    return np.array(rows, dtype=object).reshape(-1, 5)


def check(eng, res, ref):
    d, t = eng.unpack_decisions(res.decisions), eng.unpack_throttle(res.throttle)
    for j, f in enumerate(("status", "allowed", "remaining", "reset_after_ns", "retry_after_ns")):
        want = ref[:, j].astype(np.int64)
        assert np.array_equal(d[f].astype(np.int64), want), f
        got_t = t[f.replace("_ns", "_s")]
        assert np.array_equal(got_t, want // 10**9 if f.endswith("_ns") else want), "throttle " + f
    a, s = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (res.allowed, res.status))
    assert np.array_equal(a, d["allowed"]) and np.array_equal(s, d["status"])


def state(eng, probe_key=None):
    s = [eng.counters(), eng.read_state(0, eng.capacity), eng.sweep_stats()["operations"], eng.top_denied(50), eng.selfcheck()]
    return s + ([eng.debug_check_keys(), eng.lookup_slot(probe_key)] if probe_key is not None else [])


def same_state(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) if isinstance(x, tuple) else x == y for x, y in zip(a, b))


def key_world():
    """engine + mirror after: ~3 000 keys bound over three batches, a sweep (tombstones), some swept keys bound again"""
    uni = sorted({(b"%07d" % j + b"k" * 200)[:LENS[j % 13]] if LENS[j % 13] != 1 else bytes([j // 13 % 256]) for j in range(3500)})
    eng, orc = t.Engine(4096, 4096, key_mode=True, track_denied=True), O.AdaptiveOracle(capacity=100000, created_ns=T0, auto_cleanup=False)
    rng = np.random.default_rng(5)
    seen, short = uni[:3000], uni[:3000][1::2]  # every other key gets the plan whose entries expire within a second
    def apply(keys, now):
        kb, ko = O.pack_keys(keys)
        pl = np.array([PLANS[1] if k in shortset else PLANS[0] for k in keys])
        q = rng.integers(1, 4, len(keys))  # (a key's first request is allowed under both plans; the repeated keys meet denials)
        ref = orc.batch_keys(kb, ko, pl[:, 0], pl[:, 1], pl[:, 2], q, now)
        res = eng.rate_limit_batch_keys(kb, ko, max_burst=pl[:, 0], count_per_period=pl[:, 1], period=pl[:, 2], quantity=q, now_ns=now)
        assert all(np.array_equal(getattr(res, f).astype(np.int64), getattr(ref, f).astype(np.int64)) for f in ref.fields())
    shortset = set(short)
    for b in range(3):
        apply(seen[b * 1000:(b + 1) * 1000] + seen[:50], T0 + b * 10**9)
    orc.force_cleanup(T0 + 3 * 10**9)
    assert eng.sweep_expired(T0 + 3 * 10**9) > 1000 and len(orc) < 1700
    again = short[:100]
    shortset -= set(again[:50])  # 50 come back live, 50 with the short plan: bound but expired by the time of the peeks
    apply(again, T0 + 4 * 10**9)
    classes = {"live": seen[0::2] + again[:50], "expired": again[50:], "swept": short[100:], "never": uni[3000:]}
    return eng, orc, classes, {k: c for c in classes for k in classes[c]}


@pytest.fixture(scope="module")
def world():
    w = key_world()
    yield w
    w[0].close()


def peek_keys_case(eng, orc, classes, cls_of, n, dev, form, only=None, seed=0):
    rng = np.random.default_rng(seed + n)
    names = [only] * n if only else list(rng.choice(list(classes), n))
    keys = [classes[c][rng.integers(len(classes[c]))] for c in names]
    keys[n // 2:] = keys[:n - n // 2] if n > 8 else keys[n // 2:]  # duplicates
    if n > 8:  # the arena ends with a 113-byte key, or with one that fits an entry
        keys[-1] = [k for k in classes["never"] if len(k) == (113 if n % 2 == 0 else 9)][0]
    names = [cls_of[k] for k in keys]
    pid = rng.integers(0, 3, n) if form != "scalars" else np.zeros(n, np.int64)
    if form != "scalars" and n > 8:
        pid[3] = 3                                         # one invalid triple
    pl = np.array(PLANS)[pid]
    q = np.array([(0, 1, b, b + 1)[j % 4] for j, b in enumerate(pl[:, 0])], np.int64)
    if form != "dict" and n > 8:
        q[5] = -2                                          # one negative quantity (quantity32 cannot carry one)
    now = T0 + 6 * 10**9 + (np.arange(n) % 3) * 10**8
    ref = reference(orc.get, keys, pl[:, 0], pl[:, 1], pl[:, 2], q, now)
    if n > 8:  # the case is not vacuous: said by the reference and by how the world was made
        assert set(names) == set(classes) and set(ref[:, 1]) == {0, 1}
        assert set(ref[:, 0]) == {0} | ({1} if form != "dict" else set()) | ({2} if form != "scalars" else set())
        assert all((orc.get(k, int(t)) is not None) == (c == "live") for k, c, t in zip(keys, names, now))
    kb, ko = O.pack_keys(keys)
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: a)
    kw = dict(now_ns=up(now), want=eng.PEEK_FIELDS)
    if form == "dict":
        kw.update(plan_dict=(up(np.array(PLANS, np.int64)), up(pid.astype(np.uint16).view(np.int16) if dev else pid.astype(np.uint16)),
                             up(q.astype(np.uint32).view(np.int32) if dev else q.astype(np.uint32))))
    elif form == "columns":
        kw.update(max_burst=up(pl[:, 0].copy()), count_per_period=up(pl[:, 1].copy()), period=up(pl[:, 2].copy()), quantity=up(q))
    else:
        kw.update(max_burst=5, count_per_period=10, period=60, quantity=up(q))
    res = eng.peek_batch_keys(up(kb), up(ko.astype(np.int32)) if dev else ko, **kw)
    eng.synchronize()
    check(eng, res, ref)


CASES = [(n, dev, form, None) for n in (255, 256, 257, 1500) for dev in (False, True) for form in ("scalars", "columns", "dict")]
CASES += [(1, c != "swept", "columns", c) for c in ("live", "expired", "swept", "never")]


@pytest.mark.parametrize("n,dev,form,only", CASES)
def test_peek_keys_every_class(world, n, dev, form, only):
    peek_keys_case(*world, n, dev, form, only)


@pytest.mark.parametrize("n", [1500, 20000])  # (every TC_B_INPUTS_READY key batch takes the key stream: keys.hip has no size threshold)
def test_peek_between_pipelined_key_batches(n):
    eng, orc = t.Engine(4 * n, n, key_mode=True), O.AdaptiveOracle(capacity=100000, created_ns=T0, auto_cleanup=False)
    eng.use_torch_stream()
    k1, k2 = [b"one:%d" % j for j in range(n // 2)], [b"two-with-a-longer-key:%d" % j for j in range(n // 2)]
    rng = np.random.default_rng(n)
    mix = lambda ks: [ks[j] for j in rng.integers(0, len(ks), n)]
    batches = [mix(k1), mix(k1 + k2), mix(k2 + k1[:10])]
    dev = [[torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).cuda() for a in O.pack_keys(b)] for b in batches]
    torch.cuda.synchronize()
    plan = dict(max_burst=3, count_per_period=10, period=1, quantity=1)
    a = eng.rate_limit_batch_keys(*dev[0], now_ns=T0, inputs_ready=True, **plan)
    p = eng.peek_batch_keys(*dev[1], now_ns=T0 + 10**8, want=eng.PEEK_FIELDS, **plan)
    b = eng.rate_limit_batch_keys(*dev[2], now_ns=T0 + 2 * 10**8, inputs_ready=True, **plan)
    eng.sweep_expired_async(T0 + 10**9)
    eng.synchronize()
    ra = orc.batch_keys(*O.pack_keys(batches[0]), 3, 10, 1, 1, T0)
    rp = reference(orc.get, batches[1], *(np.full(n, v) for v in (3, 10, 1, 1, T0 + 10**8)))
    rb = orc.batch_keys(*O.pack_keys(batches[2]), 3, 10, 1, 1, T0 + 2 * 10**8)
    size = len(orc)
    orc.force_cleanup(T0 + 10**9)
    check(eng, p, rp)
    for res, ref in ((a, ra), (b, rb)):
        assert all(np.array_equal(getattr(res, f).cpu().numpy().astype(np.int64), getattr(ref, f).astype(np.int64)) for f in ref.fields())
    assert eng.counters()["swept"] == size - len(orc) > 0 and eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    eng.close()


@pytest.mark.parametrize("fixed,registered", [(False, True), (False, False), (True, True)])
@pytest.mark.parametrize("dev", [False, True])
def test_peek_slots(fixed, registered, dev):
    cap, n = 4096, 1500
    eng, orc = t.Engine(cap, 4096, fixed_params=fixed, track_denied=True), O.DenseOracle(cap)
    tier = np.array(PLANS[:2])[np.arange(cap) % 2]  # slot -> (burst, count, period); odd slots expire within a second
    if fixed:  # a peek before the first batch seals nothing: the plans can still be registered after it
        eng.register_params_uniform(7, 7, 7)
        eng.peek_batch_slots(np.arange(10), registered=True, quantity=1, now_ns=T0)
    eng.register_params(tier[:, 0], tier[:, 1], tier[:, 2])
    rng = np.random.default_rng(3)
    for b, now in enumerate((T0, T0 + 10**9)):  # slots < 3000 get written; a sweep at +3 s vacates the odd ones; 100 odd ones come back
        sl = rng.integers(0, 3000, 3000).astype(np.uint32)
        q = rng.integers(1, 7, sl.size)
        orc.batch_slots(sl, tier[sl, 0], tier[sl, 1], tier[sl, 2], q, now)
        eng.rate_limit_batch_slots(sl, registered=True, quantity=q, now_ns=now)
    assert eng.sweep_expired(T0 + 3 * 10**9) == orc.sweep(T0 + 3 * 10**9) > 500
    sl = np.arange(1, 201, 2, dtype=np.uint32)
    orc.batch_slots(sl, tier[sl, 0], tier[sl, 1], tier[sl, 2], 1, T0 + 4 * 10**9)
    eng.rate_limit_batch_slots(sl, registered=True, quantity=1, now_ns=T0 + 4 * 10**9)
    tat, exp, occ = orc.dump()
    get = lambda s, now: int(tat[s]) if occ[s] and int(exp[s]) > now else None
    slots = rng.integers(0, cap, n).astype(np.uint32)
    slots[:400] = rng.integers(0, 200, 400)
    pl = tier[slots] if registered else np.array(PLANS)[rng.integers(0, 4, n)]
    q = np.array([(0, 1, b, b + 1)[j % 4] for j, b in enumerate(pl[:, 0])], np.int64)
    q[7] = -1
    now = T0 + 6 * 10**9 + (np.arange(n) % 3) * 10**8
    ref = reference(get, slots, pl[:, 0], pl[:, 1], pl[:, 2], q, now)
    live = np.array([get(s, int(w)) is not None for s, w in zip(slots, now)])
    assert live.any() and (occ[slots] & ~live).any() and (~occ[slots] & (slots < 3000)).any() and (slots >= 3000).any() and set(ref[:, 1]) == {0, 1}
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: a)
    kw = {} if registered else dict(max_burst=up(pl[:, 0].copy()), count_per_period=up(pl[:, 1].copy()), period=up(pl[:, 2].copy()))
    before = state(eng)
    res = eng.peek_batch_slots(up(slots.view(np.int32)) if dev else slots, registered=registered, quantity=up(q), now_ns=up(now), want=eng.PEEK_FIELDS, **kw)
    eng.synchronize()
    check(eng, res, ref)
    assert same_state(before, state(eng))
    eng.close()


def test_refusals_enqueue_nothing(world):
    eng = world[0]
    before = eng.counters()
    kb, ko, out = np.frombuffer(b"abcd", np.uint8).copy(), np.array([0, 2, 4], np.uint32), np.zeros(12, np.uint32)
    at = out.ctypes.data + (-out.ctypes.data % 16)
    def call(flags=0, o=at, keys=True, e=eng, **fields):
        b = L.tc_batch(struct_size=C.sizeof(L.tc_batch), flags=flags, n=2, key_bytes=kb.ctypes.data, key_off=ko.ctypes.data, slot=ko.ctypes.data,
                       max_burst_scalar=5, count_per_period_scalar=10, period_scalar=60, quantity_scalar=1, now_ns_scalar=T0, **fields)
        rc = (e._lib.tc_peek_batch_keys if keys else e._lib.tc_peek_batch_slots)(e._h, C.byref(b), o)
        return rc, e._lib.tc_last_error(e._h).decode()
    assert call()[0] == 0
    for flag, word in ((L.TC_B_ASYNC, "TC_B_ASYNC"), (L.TC_B_GROUPED_OUTPUT, "TC_B_GROUPED_OUTPUT"), (L.TC_B_UNIQUE_SLOTS, "TC_B_UNIQUE_SLOTS")):
        rc, msg = call(flag)
        assert rc == L.TC_E_UNSUPPORTED and word in msg and "tc_peek_batch_keys" in msg
    assert call(n_segments=1)[0] == L.TC_E_UNSUPPORTED and call(o=None)[0] == L.TC_E_INVALID_ARG and "no output" in call(o=None)[1]
    assert call(o=at + 4)[0] == call(limit=at)[0] == call(keys=False)[0] == L.TC_E_INVALID_ARG
    slot_eng = t.Engine(64, 64)
    rc, msg = call(e=slot_eng)
    assert rc == L.TC_E_UNSUPPORTED and "TC_CFG_KEY_MODE" in msg
    assert slot_eng.counters()["total"] == 0 and eng.counters() == before
    slot_eng.close()


def test_peeks_change_nothing_and_later_batches_do_not_notice(world):  # (last: it ends with a real batch)
    eng, orc, classes, cls_of = world
    probe = classes["never"][0]
    before = state(eng, probe)
    for dev in (False, True):
        peek_keys_case(eng, orc, classes, cls_of, 1500, dev, "columns", seed=dev)
    assert same_state(before, state(eng, probe))
    keys = [classes[c][j] for c in classes for j in range(40)]
    kb, ko = O.pack_keys(keys)
    ref = orc.batch_keys(kb, ko, 5, 10, 60, 2, T0 + 7 * 10**9)
    res = eng.rate_limit_batch_keys(kb, ko, max_burst=5, count_per_period=10, period=60, quantity=2, now_ns=T0 + 7 * 10**9)
    assert all(np.array_equal(getattr(res, f).astype(np.int64), getattr(ref, f).astype(np.int64)) for f in ref.fields())
