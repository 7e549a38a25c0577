"""tc_route_keys: a string-key arena in device memory partitioned by owning GPU -- against tc_route_keys_host's owners and
plain numpy indexing, and end to end through two key-mode engines against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import kat

pytestmark = pytest.mark.gpu

LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 112, 113, 300)  # every hash path, both sides of each boundary
SENT = 0x5A5A5A5A
FIELDS = ("allowed", "limit", "remaining", "reset_after_ns", "retry_after_ns", "status")


def _arena(case):
    """-> (key_bytes uint8, key_off uint32[n + 1])"""
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    if case == "one":
        keys = [b"k"]
    elif case == "long":  # 1 100 keys of 300 bytes, one of them 5 000: no tile fits the staging buffer
        keys = [rng.integers(0, 256, 300, dtype=np.uint8).tobytes() for _ in range(1100)]
        keys[700] = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    else:  # 12 325 keys: the lengths cycle, every fifth key repeats an earlier one, the last one is short
        keys = []
        for i in range(12325):
            keys.append(keys[int(rng.integers(0, i))] if i % 5 == 4 else rng.integers(0, 256, LENS[i % len(LENS)], dtype=np.uint8).tobytes())
        keys[-1] = b"end"
    return O.pack_keys(keys)


@pytest.fixture(scope="module")
def arenas():
    import torch
    out = {}
    for case in ("main", "long", "one"):
        kb, ko = _arena(case)
        out[case] = (kb, ko, torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda())
    return out


def _segment(kb, ko, owner, d):
    """destination d's arena by numpy indexing -> (offsets, bytes, positions)"""
    pos = np.nonzero(owner == d)[0]
    lens = (ko[pos + 1] - ko[pos]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(ko[pos].astype(np.int64) - off[:-1], lens) + np.arange(off[-1])
    return off, kb[idx], pos


def _outputs(torch, total, n, world):
    """sentinel-filled (bytes, off, pos, counts) with room behind the defined layout"""
    return (torch.full((total + 64,), SENT & 0xFF, dtype=torch.uint8, device="cuda"), torch.full((n + world + 8,), SENT, dtype=torch.int32, device="cuda"),
            torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda"), torch.full((2 * world,), SENT, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("case", ["main", "long", "one"])
def test_partition_equals_the_hosts(arenas, case, world):
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import sharded
    kb, ko, d_kb, d_ko = arenas[case]
    n, total = len(ko) - 1, int(ko[-1])
    owner = sharded.route_keys(kb, ko, world)
    segs = [_segment(kb, ko, owner, d) for d in range(world)]
    counts = np.array([len(s[2]) for s in segs] + [s[0][-1] for s in segs], dtype=np.int64)
    eng = t.Engine(1000, 1000)  # (any engine: the router never touches a key table)
    host = eng.host_alloc(2 * world + 1, np.uint32)
    for tag, only in enumerate(sorted({-1, 0, world - 1}), start=1):
        outs = _outputs(torch, total, n, world)
        torch.cuda.synchronize()
        eng.route_keys(d_kb, d_ko, world, only=only, out=outs, host_counts=host, tag=tag)
        eng.synchronize()
        ob, oo, op, oc = (x.cpu().numpy() for x in outs)
        assert np.array_equal(oc.astype(np.int64), counts) and np.array_equal(host[:-1].astype(np.int64), counts) and host[-1] == tag
        k0 = b0 = 0
        for d in ([only] if only >= 0 else range(world)):
            off, byt, pos = segs[d]
            o0 = k0 + (d if only < 0 else 0)
            assert np.array_equal(oo[o0: o0 + len(pos) + 1], off), (only, d)
            assert np.array_equal(ob[b0: b0 + off[-1]], byt), (only, d)
            assert np.array_equal(op[k0: k0 + len(pos)], pos), (only, d)
            k0, b0 = k0 + len(pos), b0 + off[-1]
        # nothing beyond the defined layout was written
        assert (ob[b0:] == SENT & 0xFF).all() and (oo[k0 + (world if only < 0 else 1):] == SENT).all() and (op[k0:] == SENT).all()
    eng.close()


def test_two_key_mode_engines_answer_like_one_store():
    import torch
    import throttlecrab_amd as t
    from oracle import oracle as O
    from throttlecrab_amd import sharded
    t0 = kat.load()["t0_ns"]
    rng = np.random.default_rng(3)
    keys = [b"key_%d" % i if i % 3 else rng.integers(33, 127, LENS[i % len(LENS)], dtype=np.uint8).tobytes() + b"#%d" % i for i in range(200)]
    engs = [t.Engine(4096, 1 << 16, key_mode=True) for _ in range(2)]
    orc = O.AdaptiveOracle(capacity=100000, created_ns=t0, auto_cleanup=False)
    for b in range(3):
        n = 1500
        kb, ko = O.pack_keys([keys[i] for i in np.minimum(rng.zipf(1.3, n) - 1, len(keys) - 1)])
        now = t0 + b * 700_000_000
        ref = orc.batch_keys(kb, ko, 10, 100, 60, 1, now)
        segs, counts = sharded.split_keys_device(engs[0], torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda(), n, 2)
        assert int(counts[0]) + int(counts[1]) == n and min(counts[:2]) > 0
        got = {f: np.zeros(n, np.int64) for f in FIELDS}
        for d, (byt, off, pos) in enumerate(segs):  # straight from the router's outputs
            res = engs[d].rate_limit_batch_keys(byt, off, max_burst=10, count_per_period=100, period=60, quantity=1, now_ns=now)
            engs[d].synchronize()
            for f in FIELDS:
                got[f][pos.cpu().numpy()] = getattr(res, f).cpu().numpy().astype(np.int64)
        for f in FIELDS:
            assert np.array_equal(got[f], getattr(ref, f).astype(np.int64)), (b, f)
    for e in engs:
        assert e.selfcheck() == 0
        e.close()


@pytest.mark.parametrize("bad", [dict(world=0), dict(world=65), dict(only=2), dict(flags=1), dict(out_off=None)])
def test_bad_arguments_are_refused_with_nothing_written(arenas, bad):
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import _lib as L
    kb, ko, d_kb, d_ko = arenas["main"]
    n, world = len(ko) - 1, 2
    outs = _outputs(torch, int(ko[-1]), n, 64)
    torch.cuda.synchronize()
    eng = t.Engine(1000, 1000)
    r = L.tc_key_route(struct_size=C.sizeof(L.tc_key_route), world=world, n=n, key_bytes=d_kb.data_ptr(), key_off=d_ko.data_ptr(), only=-1,
                       out_bytes=outs[0].data_ptr(), out_off=outs[1].data_ptr(), out_pos=outs[2].data_ptr(), out_count=outs[3].data_ptr())
    for k, v in bad.items():
        setattr(r, k, v)
    assert eng._lib.tc_route_keys(eng._h, C.byref(r)) == L.TC_E_INVALID_ARG
    eng.synchronize()
    torch.cuda.synchronize()
    assert (outs[0] == SENT & 0xFF).all() and all((x == SENT).all() for x in outs[1:])
    eng.close()
