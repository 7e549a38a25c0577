"""tc_forget_batch: named keys / slots leave a live engine.  The reference has no remove, so the plain reference for "forgotten" is
a RENAME: the CPU oracle is fed the same stream with every request for a forgotten key after the forget presented under a fresh
name the stream never uses (keys: one byte appended; slots: s + CAP in a model of 2 * CAP) -- a never-seen key is exactly what a
forgotten key must be.  Integer-exact."""
import ctypes as C

import numpy as np
import pytest

from tests import kat

pytestmark = pytest.mark.gpu

FIELDS = ("allowed", "limit", "remaining", "reset_after_ns", "retry_after_ns", "status")
LENS = (1, 9, 16, 17, 64, 112, 113, 300)  # inline in the entry (<= 16), in the KeyRec (<= 112), in the overflow arena
PLANS = np.array([[5, 10, 60], [2, 100, 10], [50, 10, 60]])  # entries stay ~30 s, ~0.2 s, ~300 s: one second later some have expired
S, CAP = 10**9, 2000


def _keys(n):
    pad = np.random.default_rng(5).integers(0, 255, 300, dtype=np.uint8).tobytes()  # (no 0xFF: the renamed keys end in one)
    return list(dict.fromkeys((b"%d:" % i + pad)[:LENS[i % len(LENS)]] for i in range(n)))


def _same(res, ref, what):
    for f in FIELDS:
        got = getattr(res, f)
        assert np.array_equal((got.cpu().numpy() if hasattr(got, "cpu") else got).astype(np.int64), getattr(ref, f).astype(np.int64)), (what, f)


def _plans(ids):
    return tuple(np.ascontiguousarray(PLANS[np.asarray(ids) % 3, k]) for k in range(3))


@pytest.mark.parametrize("track_denied", [False, True])
def test_key_mode_parity(track_denied):
    import throttlecrab_amd as t
    from oracle import oracle as O
    t0, rng, keys = kat.load()["t0_ns"], np.random.default_rng(1), _keys(300)
    nk = len(keys)
    eng = t.Engine(nk, 4096, key_mode=True, track_denied=track_denied)  # full after batch 1
    orc = O.AdaptiveOracle(capacity=100000, created_ns=t0, auto_cleanup=False)
    name = {i: keys[i] for i in range(nk)}  # what the model calls key i

    def batch(ids, now, what):
        b, c, p = _plans(ids)
        kb, ko = O.pack_keys([keys[i] for i in ids])
        ref = orc.batch_keys(*O.pack_keys([name[i] for i in ids]), b, c, p, 1, now)
        _same(eng.rate_limit_batch_keys(kb, ko, max_burst=b, count_per_period=c, period=p, quantity=1, now_ns=now), ref, what)  # (raises TC_E_TABLE_FULL)
        return ref

    ids1 = np.concatenate([np.arange(nk), rng.integers(0, nk, 3000)])
    ref1 = batch(ids1, t0, "batch 1")
    assert len(set(ref1.allowed)) == 2 and eng.counters()["live_slots"] == nk
    gone = np.arange(nk // 3)
    asked = [keys[i] for i in np.concatenate([gone, gone[::4]])] + [b"never-seen-%d" % i for i in range(10)] + [keys[0]]
    want_live = np.array([orc.get(k, t0 + S) is not None for k in asked])
    n_live = sum(orc.get(keys[i], t0 + S) is not None for i in gone)
    assert 0 < n_live < len(gone)
    kb, ko = O.pack_keys(asked)
    cnt, live = eng.forget_batch(len(asked), t0 + S, key_bytes=kb, key_off=ko, was_live=True)
    assert cnt.tolist() == [len(gone), n_live] and np.array_equal(live.astype(bool), want_live)
    assert all(eng.lookup_slot(keys[i]) == -1 for i in gone) and eng.lookup_slot(keys[len(gone)]) >= 0
    assert eng.counters()["live_slots"] == nk - len(gone) and eng.debug_check_keys() == 0
    if track_denied:  # the denials stay with the KEY (keys over 256 bytes are not kept, like the reference's metrics)
        denied = {i: int(((ids1 == i) & (ref1.status == 0) & (ref1.allowed == 0)).sum()) for i in gone if len(keys[i]) <= 256}
        top = dict(eng.top_denied(1000))
        assert any(denied.values()) and all(top.get(keys[i], 0) == d for i, d in denied.items())
    name.update({i: keys[i] + b"\xff" for i in gone})
    batch(np.concatenate([np.arange(nk), rng.integers(0, nk, 1000)]), t0 + 2 * S, "batch 2")
    assert eng.counters()["live_slots"] == nk and eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    eng.close()


@pytest.mark.parametrize("fixed", [False, True])
def test_slot_mode_parity(fixed):
    import throttlecrab_amd as t
    from oracle import oracle as O
    t0, rng = kat.load()["t0_ns"], np.random.default_rng(2)
    eng, orc = t.Engine(CAP, 4096, fixed_params=fixed), O.DenseOracle(2 * CAP)
    if fixed:  # a forget decides nothing: the plans are not sealed by it
        assert eng.forget_batch(3, t0, slot=np.array([0, 1, CAP], np.uint32))[0].tolist() == [0, 0]
    eng.register_params(*_plans(np.arange(CAP)))
    name = np.arange(CAP)

    def batch(slots, now, what):
        ref = orc.batch_slots(name[slots], *_plans(slots), 1, now)
        _same(eng.rate_limit_batch_slots(slots.astype(np.uint32), registered=True, quantity=1, now_ns=now), ref, what)

    batch(rng.integers(0, CAP, 3000), t0, "batch 1")
    _, exp, occ = orc.dump(0, CAP)
    gone = np.arange(900)  # with the duplicates: more than one block of either kernel
    asked = np.concatenate([gone, gone[::3], [CAP, CAP + 5, 2**32 - 1]]).astype(np.uint32)
    want_live = np.array([s < CAP and exp[s] > t0 + S for s in asked])
    cnt, live = eng.forget_batch(len(asked), t0 + S, slot=asked, was_live=True)
    assert cnt.tolist() == [int(occ[gone].sum()), int(want_live[:len(gone)].sum())] and 0 < cnt[1] < cnt[0] < len(gone)
    assert np.array_equal(live.astype(bool), want_live)
    tat, exp = eng.read_state(0, CAP)
    assert not tat[gone].any() and not exp[gone].any() and np.count_nonzero(exp[len(gone):]) == int(occ[len(gone):].sum())
    name[gone] += CAP
    batch(rng.integers(0, CAP, 3000), t0 + 2 * S, "batch 2")
    assert eng.selfcheck() == 0
    eng.close()


def test_ordering_without_host_synchronisation():
    import torch
    import throttlecrab_amd as t
    from oracle import oracle as O
    t0, keys = kat.load()["t0_ns"], _keys(600)
    dev = lambda kb, ko: (torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda())
    a, f, b = dev(*O.pack_keys(keys[:400] * 3)), dev(*O.pack_keys(keys[100:300] + keys[500:])), dev(*O.pack_keys(keys * 3))
    got = []
    for sync in (False, True):
        eng = t.Engine(1000, 4096, key_mode=True)
        eng.rate_limit_batch_keys(*dev(*O.pack_keys(keys[300:350])), max_burst=5, count_per_period=10, period=60, quantity=1, now_ns=t0)
        eng.synchronize()  # (the side streams exist now; nothing below waits in the first round)
        out = []
        for step, (kb, ko) in enumerate((a, f, b)):
            if step == 1:
                out.append(eng.forget_batch(ko.numel() - 1, t0 + S, key_bytes=kb, key_off=ko, was_live=True))
            else:
                out.append(eng.rate_limit_batch_keys(kb, ko, max_burst=5, count_per_period=10, period=60, quantity=1, now_ns=t0 + step * S, inputs_ready=True))
            if sync:
                eng.synchronize()
        eng.synchronize()
        tat, exp = eng.read_state(0, 1000)
        assert all(eng.lookup_slot(k) >= 0 for k in keys[100:300:7]) and eng.debug_check_keys() == 0 and eng.selfcheck() == 0
        got.append([getattr(r, fld).cpu().numpy() for r in (out[0], out[2]) for fld in FIELDS] + [out[1][0].cpu().numpy(), out[1][1].cpu().numpy(),
                                                                                                  np.sort(tat), np.sort(exp)])
        eng.close()
    assert got[0][-4].tolist() == [200, 200] and all(np.array_equal(x, y) for x, y in zip(*got))


@pytest.mark.parametrize("key_mode,bad", [(True, dict(struct_size=8)), (True, dict(flags=1)), (False, dict(n=0)), (True, dict(n=65)), (False, dict(out_count=None)),
                                          (True, dict(key_bytes=None)), (True, dict(key_off=None)), (False, dict(slot=None))])
def test_refusals_change_nothing(key_mode, bad):
    import torch
    import throttlecrab_amd as t
    from oracle import oracle as O
    from throttlecrab_amd import _lib as L
    t0, keys = kat.load()["t0_ns"], _keys(64)
    eng = t.Engine(64, 64, key_mode=key_mode)
    buf = {k: torch.zeros(512, dtype=dt, device="cuda") for k, dt in (("slot", torch.int32), ("key_bytes", torch.uint8), ("key_off", torch.int32), ("out_count", torch.int64))}
    f = L.tc_forget(struct_size=C.sizeof(L.tc_forget), n=8, now_ns=t0, **{k: v.data_ptr() for k, v in buf.items()})
    for k, v in bad.items():
        setattr(f, k, v)
    with pytest.raises(t.TcError) as ei:
        eng._check(eng._lib.tc_forget_batch(eng._h, C.byref(f)))
    assert ei.value.code == L.TC_E_INVALID_ARG
    ids, plan = np.arange(64) % 16, dict(max_burst=2, count_per_period=10, period=60, quantity=1, now_ns=t0)
    if key_mode:
        kb, ko = O.pack_keys([keys[i] for i in ids])
        res, ref = eng.rate_limit_batch_keys(kb, ko, **plan), O.AdaptiveOracle(created_ns=t0, auto_cleanup=False).batch_keys(kb, ko, 2, 10, 60, 1, t0)
    else:
        res, ref = eng.rate_limit_batch_slots(ids.astype(np.uint32), **plan), O.DenseOracle(64).batch_slots(ids, 2, 10, 60, 1, t0)
    _same(res, ref, bad)
    assert len(set(ref.allowed)) == 2 and eng.selfcheck() == 0
    eng.close()
