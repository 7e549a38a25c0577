"""The string-key table on keys that share a full 64-bit hash (tests/keysteer.py builds them): every place that confirms a hit by
the key's bytes -- bound entries of each length class, pending claims of the same batch, the single-request path, the table of
retired denial counts -- is walked with "hash equal, key different" on both sides of 16 / 64 / 112 bytes, with chosen homes (a
chain over the table's end), chosen tags, and chosen owners for tc_route_keys.  The reference is the CPU oracle, which keys on
the bytes and knows nothing of this hash; every comparison is exact."""
import collections
import functools

import numpy as np
import pytest

from tests import keysteer as ks

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000 * 10**9
S = 10**9
FIELDS = ("allowed", "limit", "remaining", "reset_after_ns", "retry_after_ns", "status")
TWIN_LENS = (9, 12, 16, 17, 40, 64, 65, 112, 113, 200)  # Entry::key | words in KeyRec | bytes in KeyRec | overflow arena
CROSS_LENS = (24, 32, 72, 120, 200)
CROWD_LENS = (9, 16, 17, 33, 64, 65, 112, 113, 130)
LONG, SHORT, DENY = (5, 10, 60), (3, 10, 1), (3, 10, 60)     # SHORT: entries expire within a second
CAP = 2048


class Families:
    """twins[g]: 4 keys of one length with one hash + 2 spares (members 4, 5) for the scenarios that need a newcomer;
    cross[g]: 5 keys of different lengths, one hash, each a prefix of the next; near[kind]: pairs; crowd: 200 keys at home nb - 3"""

    def __init__(self, nb):
        rng = np.random.default_rng(20240607)
        self.nb = nb
        self.twins = [ks.twins(n, 6, rng) for n in TWIN_LENS for _ in range(6)]
        self.cross = [ks.cross_length(CROSS_LENS, rng) for _ in range(6)]
        mk = lambda n, h: ks.steer(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), h, ks.steer_word(n))
        self.near = {"tag": [], "home": [], "bit63": []}
        for j in range(8):
            n, pos, tag = TWIN_LENS[j], int(rng.integers(0, nb)), int(rng.integers(0, 1 << 24))
            self.near["tag"].append([mk(n, ks.home_hash(pos, nb, rng, tag)) for _ in range(2)])     # one home, one tag, two hashes
            self.near["home"].append([mk(n, ks.home_hash(pos + 1 & nb - 1, nb, rng, tag ^ m)) for m in (0, 1 + j)])  # one home, two tags
            h = ks.home_hash(int(rng.integers(0, nb)), nb, rng)
            self.near["bit63"].append([mk(n, h), mk(n, h ^ ks.RT_VALID)])  # one retired-table tag and home; the key table's tags differ
        one = ks.home_hash(nb - 3, nb, rng)
        self.crowd = [ks.at_home(nb - 3, nb, rng, CROWD_LENS[j % 9]) for j in range(160)]
        self.crowd += [mk((12, 40, 113, 200)[j % 4], one) for j in range(40)]  # 40 of them twins of each other
        self.check()

    def groups(self, members=4):
        """every group as a list of keys (twins cut to `members`); the crowd counts as one group"""
        return [g[:members] for g in self.twins] + self.cross + [p for ps in self.near.values() for p in ps] + [self.crowd]

    def keys(self, members=4):
        return [k for g in self.groups(members) for k in g]

    def check(self):
        """the families are what the scenarios need, from the helper's own hashes: not one scenario below is vacuous"""
        nb, H = self.nb, ks.hash_key
        for n in TWIN_LENS:  # every length class has groups of unequal keys with ONE hash
            gs = [g for g in self.twins if len(g[0]) == n]
            assert len(gs) == 6 and all(len(set(g)) == 6 and len({H(k) for k in g}) == 1 and {len(k) for k in g} == {n} for g in gs)
        assert all(len({H(k) for k in g}) == 1 and [len(k) for k in g] == list(CROSS_LENS) and g[4].startswith(g[0]) for g in self.cross)
        tag = lambda k: H(k) >> 40
        home = lambda k: H(k) & (nb - 1)
        for a, b in self.near["tag"]:
            assert home(a) == home(b) and tag(a) == tag(b) and H(a) != H(b) and len(a) == len(b)
        for a, b in self.near["home"]:
            assert home(a) == home(b) and tag(a) != tag(b)
        for a, b in self.near["bit63"]:
            assert H(a) ^ H(b) == 1 << 63 and H(a) | ks.RT_VALID == H(b) | ks.RT_VALID and a != b and len(a) == len(b)
            assert (H(a) >> 17) % ks.RETIRED_CAP == (H(b) >> 17) % ks.RETIRED_CAP
        assert len(self.crowd) == 200 > 3 and {home(k) for k in self.crowd} == {nb - 3} and len({H(k) for k in self.crowd[160:]}) == 1
        assert len(set(self.crowd)) == 200 and len({H(k) for k in self.crowd}) == 161
        ks_all = self.keys(6)
        assert len(set(ks_all)) == len(ks_all)
        # at most 64 keys per home of the retired table (half of RETIRED_PROBES = 128): no denial count is ever dropped for want of room
        assert max(collections.Counter((H(k) >> 17) % ks.RETIRED_CAP for k in ks_all).values()) <= 64


@functools.lru_cache(maxsize=None)
def families(nb):
    return Families(nb)


def new_pair(cap=CAP, **kw):
    import throttlecrab_amd as t
    from oracle import oracle as O
    return t.Engine(cap, 8192, key_mode=True, **kw), O.AdaptiveOracle(capacity=100000, created_ns=T0, auto_cleanup=False)


def columns(keys, plan_of):
    """per-request plan columns from a function key -> (burst, count, period)"""
    pl = np.array([plan_of(k) for k in keys], np.int64)
    return pl[:, 0].copy(), pl[:, 1].copy(), pl[:, 2].copy()


def submit(eng, keys, plan, now, q=1, how="host", want=FIELDS, keep=None):
    """enqueue one batch; plan: three scalars or three columns.  how: host | device | ready (device, TC_B_INPUTS_READY).
    keep: a list that takes the input tensors of a device batch (they must outlive the batch, which is still running)"""
    import torch
    from oracle import oracle as O
    kb, ko = O.pack_keys(keys)
    if how == "host":
        return eng.rate_limit_batch_keys(kb, ko, max_burst=plan[0], count_per_period=plan[1], period=plan[2], quantity=q, now_ns=now, want=want)
    up = lambda a: a if np.ndim(a) == 0 else torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()
    args = [torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda()] + [up(a) for a in (*plan, q)]
    torch.cuda.synchronize()
    if keep is not None:
        keep.append(args)
    return eng.rate_limit_batch_keys(args[0], args[1], max_burst=args[2], count_per_period=args[3], period=args[4], quantity=args[5], now_ns=now,
                                     want=want, inputs_ready=how == "ready")


def expect(orc, keys, plan, now, q=1):
    from oracle import oracle as O
    kb, ko = O.pack_keys(keys)
    return orc.batch_keys(kb, ko, plan[0], plan[1], plan[2], q, now)


def same(res, ref, what=""):
    for f in FIELDS:
        got = getattr(res, f)
        got = (got.cpu().numpy() if hasattr(got, "cpu") else got).astype(np.int64)
        want = getattr(ref, f).astype(np.int64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, f, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def apply(eng, orc, keys, plan, now, q=1, how="host", what=""):
    ref = expect(orc, keys, plan, now, q)
    keep = []
    res = submit(eng, keys, plan, now, q, how, keep=keep)
    eng.synchronize()
    same(res, ref, what)
    return ref


def finish(eng, orc, bound, absent=()):
    """how every scenario ends: a healthy table, as many bound keys as the oracle holds, one slot per bound key"""
    eng.synchronize()
    assert eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    assert eng.counters()["live_slots"] == len(orc)
    slots = [eng.lookup_slot(k) for k in bound]
    assert min(slots) >= 0 and len(set(slots)) == len(slots), [k for k, s in zip(bound, slots) if s < 0][:3]
    assert all(eng.lookup_slot(k) == -1 for k in absent)
    return dict(zip(bound, slots))


def shuffled(keys, rng, lo=1, hi=5):
    """every key lo..hi times, in shuffled order"""
    out = [k for k in keys for _ in range(int(rng.integers(lo, hi + 1)))]
    return [out[i] for i in rng.permutation(len(out))]


# ---- 1. all new in one batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host", "device", "ready"])
def test_all_new_in_one_batch(how):
    """Twins race for one entry with equal meta words; a duplicate must follow ITS key's claimant (the pending-claim comparison
    against the claimant's bytes in the batch arena, by words and by bytes), not a twin's.  Burst 3: a shared bucket shows in
    `remaining` and in the denials.  `ready`: the second batch is enqueued behind the first without a wait (the key stream)."""
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair()
    if how != "host":
        eng.use_torch_stream()
    rng = np.random.default_rng(1)
    held = set(g[3] for g in fam.twins) | set(g[4] for g in fam.cross) | set(fam.crowd[1::2])
    first = shuffled([k for k in fam.keys() if k not in held], rng)
    second = shuffled(fam.keys(), rng, 1, 3)   # found keys, their unseen twins and duplicates of both in one batch
    assert max(len(first), len(second)) <= 6000 and min(collections.Counter(first + second).values()) >= 1
    refs = [expect(orc, first, DENY, T0), expect(orc, second, DENY, T0 + S // 10)]
    assert all(set(r.allowed) == {0, 1} for r in refs)
    keep = []
    res = [submit(eng, first, DENY, T0, how=how, keep=keep)]
    if how != "ready":
        eng.synchronize()
    res.append(submit(eng, second, DENY, T0 + S // 10, how=how, keep=keep))
    eng.synchronize()
    for j in range(2):
        same(res[j], refs[j], (how, j))
    finish(eng, orc, fam.keys())
    eng.close()


# ---- 2. bound, then a twin arrives -------------------------------------------------------------------------------------------
def test_twin_of_a_bound_key_arrives_in_a_batch():
    """probe_request's bound-entry branches: tag, length code and hash agree, the key does not (<= 16 bytes against Entry::key,
    17..64 by words, longer by bytes against the KeyRec or the overflow arena; cross-length: only KeyRec::len differs)"""
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair()
    rng = np.random.default_rng(2)
    apply(eng, orc, shuffled([g[0] for g in fam.groups()[:-1]] + fam.crowd[0::2], rng, 2, 4), DENY, T0, what="member 0")
    slots = finish(eng, orc, [g[0] for g in fam.groups()])
    ref = apply(eng, orc, shuffled(fam.keys(), rng, 1, 3), DENY, T0 + S // 10, what="members 0-3")
    assert set(ref.allowed) == {0, 1}
    after = finish(eng, orc, fam.keys())
    assert all(after[k] == s for k, s in slots.items())
    eng.close()


def test_twin_of_a_bound_key_arrives_alone():
    """find_or_bind_one (tc_rate_limit and the Store shims): one group per length, member 0 bound, then its twins one by one"""
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair()
    groups = [[g for g in fam.twins if len(g[0]) == n][0][:4] for n in TWIN_LENS] + fam.cross[:1] + [fam.crowd[158:164]]
    now = T0
    for g in groups:
        assert len({ks.hash_key(k) for k in g[-2:]}) == 1 and len(set(g)) == len(g)
        for rnd in range(2):
            for k in (g[:1] * 3 + g if rnd == 0 else g):
                now += 1000
                assert eng.rate_limit(k, *DENY, 2, now) == orc.rate_limit(k, *DENY, 2, now), (len(k), rnd)
        assert len({eng.lookup_slot(k) for k in g}) == len(g)
    finish(eng, orc, [k for g in groups for k in g])
    eng2, orc2 = new_pair()
    for g in groups:  # the Store shims on a fresh pair: member 0 is set, its twins must not be found, then each gets its own value
        now += 1000
        for st in (eng2, orc2):
            assert st.set_if_not_exists_with_ttl(g[0], 1000, 60 * S, now) is True
        for j, k in enumerate(g[1:], start=1):
            got = [(st.get(k, now), st.compare_and_swap_with_ttl(k, 1000, 7, 60 * S, now), st.set_if_not_exists_with_ttl(k, 1000 + j, 60 * S, now),
                    st.set_if_not_exists_with_ttl(k, 5, 60 * S, now), st.compare_and_swap_with_ttl(k, 1000 + j, 2000 + j, 60 * S, now), st.get(k, now))
                   for st in (eng2, orc2)]
            assert got[0] == got[1] == (None, False, True, False, True, 2000 + j), (len(k), j, got)
        assert [eng2.get(k, now) for k in g] == [orc2.get(k, now) for k in g] == [1000] + [2000 + j for j in range(1, len(g))]
    finish(eng2, orc2, [k for g in groups for k in g])
    eng.close()
    eng2.close()


# ---- 3. peek -----------------------------------------------------------------------------------------------------------------
def peek_reference(get, keys, plan, q, now):
    """rows of (status, allowed, remaining, reset_after_ns, retry_after_ns): PyModel.rate_limit on {key: live tat} or {} (as
    tests/test_gpu_peek.py)"""
    from oracle.pymodel import PyModel
    rows = []
    for k in keys:
        m, tat = PyModel(), get(k, now)
        if tat is not None:
            m.data[k] = (tat, now + 1)
        st, al, _, rem, rs, rt = m.rate_limit(k, *plan, q, now)
        rows.append((st, int(al), rem, rs, rt))
    return np.array(rows, dtype=object).reshape(-1, 5)


@pytest.mark.parametrize("dev", [False, True])
def test_peek_tells_twins_apart(dev):
    import torch
    from oracle import oracle as O
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair(track_denied=True)
    rng = np.random.default_rng(3)
    groups = fam.groups()
    bound = [g[0] for g in groups[:-1]] + fam.crowd[0::4]
    swept = [g[1] for g in groups[:-1]] + fam.crowd[1::4]
    never = [k for g in groups[:-1] for k in g[2:]] + fam.crowd[2::4] + fam.crowd[3::4]
    boundset = set(bound)
    first = shuffled(bound + swept, rng, 2, 4)
    apply(eng, orc, first, columns(first, lambda k: LONG if k in boundset else SHORT), T0)
    before = len(orc)
    orc.force_cleanup(T0 + 3 * S)
    assert eng.sweep_expired(T0 + 3 * S) == before - len(orc) == len(swept)
    now = T0 + 4 * S
    keys = shuffled(bound + swept + never, rng, 1, 2)
    assert all((orc.get(k, now) is not None) == (k in boundset) for k in keys)
    ref = peek_reference(orc.get, keys, LONG, 2, now)
    fresh = peek_reference(lambda k, t: None, keys[:1], LONG, 2, now)[0]
    assert all(tuple(r) == tuple(fresh) for k, r in zip(keys, ref) if k not in boundset) and any(tuple(r) != tuple(fresh) for r in ref)
    state = lambda: (eng.counters(), [a.tolist() for a in eng.read_state(0, CAP)], eng.top_denied(50), eng.selfcheck(), eng.debug_check_keys(),
                     [eng.lookup_slot(k) for k in keys[:200]])
    was = state()
    kb, ko = O.pack_keys(keys)
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: a)
    res = eng.peek_batch_keys(up(kb), up(ko.astype(np.int32)) if dev else ko, max_burst=LONG[0], count_per_period=LONG[1], period=LONG[2], quantity=2,
                              now_ns=now, want=eng.PEEK_FIELDS)
    eng.synchronize()
    d, th = eng.unpack_decisions(res.decisions), eng.unpack_throttle(res.throttle)
    for j, f in enumerate(("status", "allowed", "remaining", "reset_after_ns", "retry_after_ns")):
        want = ref[:, j].astype(np.int64)
        assert np.array_equal(d[f].astype(np.int64), want), f
        assert np.array_equal(th[f.replace("_ns", "_s")], want // S if f.endswith("_ns") else want), "throttle " + f
    assert state() == was
    finish(eng, orc, bound, absent=swept + never)
    eng.close()


# ---- 4. tombstones inside a twin chain / 6. snapshot ---------------------------------------------------------------------------
def tombstone_world(**kw):
    """Three batches bind member 1, then members 0 and 2, then member 3 of every group (chains in that order); odd members have the
    short plan and are swept at +3 s: every twin chain now STARTS with a tombstone, has live twins behind it and another
    tombstone behind those.  A newcomer (member 4) then recycles the first tombstone.  -> engine, oracle, plan_of, the time"""
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair(**kw)
    groups = fam.groups(6)
    odd = set(k for g in groups[:-1] for k in g[1:4:2]) | set(fam.crowd[1::2])
    plan_of = lambda k: SHORT if k in odd else LONG
    rng = np.random.default_rng(4)
    for j, ks_ in enumerate(([g[1] for g in groups[:-1]] + fam.crowd[1::2], [k for g in groups[:-1] for k in g[0:3:2]] + fam.crowd[0::2],
                             [g[3] for g in groups[:-1] if len(g) > 3])):
        batch = shuffled(ks_, rng, 2, 4)
        apply(eng, orc, batch, columns(batch, plan_of), T0 + j * 1000, what=("bind", j))
    before = len(orc)
    orc.force_cleanup(T0 + 3 * S)
    assert eng.sweep_expired(T0 + 3 * S) == before - len(orc) == len(odd)
    live = [k for g in groups[:-1] for k in g[0:3:2]] + fam.crowd[0::2]
    finish(eng, orc, live, absent=sorted(odd))
    newcomers = [g[4] for g in fam.twins]
    batch = shuffled(newcomers + live[::3], rng, 1, 3)
    apply(eng, orc, batch, columns(batch, plan_of), T0 + 3 * S + 1000, what="newcomer")
    finish(eng, orc, live + newcomers, absent=sorted(odd))
    return fam, eng, orc, plan_of, T0 + 3 * S + 2000


def test_tombstones_inside_a_twin_chain():
    fam, eng, orc, plan_of, now = tombstone_world()
    rng = np.random.default_rng(5)
    batch = shuffled(fam.keys(6), rng, 1, 3)   # the swept twins return, the last spare arrives, everybody else is asked again
    ref = apply(eng, orc, batch, columns(batch, plan_of), now, what="return")
    assert set(ref.allowed) == {0, 1}
    finish(eng, orc, fam.keys(6))
    eng.close()


def test_snapshot_keeps_twins_apart(tmp_path):
    from oracle import oracle as O
    fam, eng, orc, plan_of, now = tombstone_world()
    path = str(tmp_path / "twins.snap")
    eng.snapshot_save(path)
    eng.close()
    eng2, _ = new_pair()
    other = [b"other:%d" % j for j in range(1500)] + [g[5] for g in fam.twins]   # (a spare twin among them: gone after the load)
    eng2.rate_limit_batch_keys(*O.pack_keys(other), max_burst=3, count_per_period=10, period=60, quantity=1, now_ns=T0)
    eng2.snapshot_load(path)
    rng = np.random.default_rng(6)
    batch = shuffled(fam.keys(6), rng, 1, 3)
    ref = apply(eng2, orc, batch, columns(batch, plan_of), now, what="after load")
    assert set(ref.allowed) == {0, 1}
    finish(eng2, orc, fam.keys(6), absent=other[:50])
    eng2.close()


# ---- 5. rebuild --------------------------------------------------------------------------------------------------------------
def test_rebuild_reenters_colliding_keys():
    """mk::k_sweep_decide rebuilds the table when tombstones + keys just unbound > nb / 4 (the rule above k_table_clear_compact).
    1 024 slots -> nb = 2 048, nb / 4 = 512.  Live through the sweep: the crowd (200) + members 0 and 2 of the 60 twin groups
    (120) = 320.  Swept: twin members 1 and 3 (120) + the cross-length groups (30) + the near misses (48) + 400 fillers = 598
    > 512, in one sweep, with no tombstone needed from before.  320 + 598 = 918 keys <= 1 024 slots."""
    cap = 1024
    nb = ks.table_size(cap)
    fam = families(nb)
    assert nb == 2048 and ks.hash_key(fam.crowd[0]) & (nb - 1) == nb - 3
    eng, orc = new_pair(cap)
    live = fam.crowd + [k for g in fam.twins for k in g[0:3:2]]
    swept = [k for g in fam.twins for k in g[1:4:2]] + [k for g in fam.cross for k in g] + [k for ps in fam.near.values() for p in ps for k in p]
    swept += [b"filler:%d" % j for j in range(400)]
    assert len(live) == 320 and len(swept) == 598 > nb // 4 and len(live) + len(swept) <= cap
    liveset = set(live)
    plan_of = lambda k: LONG if k in liveset else SHORT
    rng = np.random.default_rng(7)
    for j, ks_ in enumerate((fam.crowd, live[200:] + swept)):  # (the crowd first: its 200 claimants race for one chain among themselves only)
        batch = shuffled(ks_, rng, 1, 3)
        apply(eng, orc, batch, columns(batch, plan_of), T0 + j * 1000, what=("bind", j))
    slots = finish(eng, orc, live + swept)
    before = len(orc)
    orc.force_cleanup(T0 + 3 * S)
    assert eng.sweep_expired(T0 + 3 * S) == before - len(orc) == len(swept)
    after = finish(eng, orc, live, absent=swept)
    assert after == {k: slots[k] for k in live}
    batch = shuffled(live + swept, rng, 1, 3)
    ref = apply(eng, orc, batch, columns(batch, plan_of), T0 + 3 * S + 1000, what="rebind")
    assert set(ref.allowed) == {0, 1}
    assert {k: s for k, s in finish(eng, orc, live + swept).items() if k in liveset} == after
    eng.close()


# ---- 7. denial counts --------------------------------------------------------------------------------------------------------
class TopDeniedModel:
    """TopDeniedKeys (throttlecrab-server/src/metrics.rs:24-76) without its size cap, as tests/test_gpu_metrics.py has it: a count
    per key, bumped on every denial; keys over 256 bytes are not tracked"""

    def __init__(self):
        self.counts = collections.Counter()

    def update(self, key):
        if len(key) <= 256:
            self.counts[key] += 1

    def get_top(self, k):
        return sorted(((key, c) for key, c in self.counts.items() if c > 0), key=lambda kv: (-kv[1], kv[0]))[:k]


def test_denial_counts_stay_with_their_key():
    """retire_denials / resurrect_denials: twins share the retired table's tag and home, and so do the pairs whose hashes differ
    in bit 63 alone (the tag is hash | 1 << 63); only the length and the bytes tell them apart.  Every member is denied a
    different number of times; the counts must follow the KEYS through three sweeps and two returns."""
    fam = families(ks.table_size(CAP))
    eng, orc = new_pair(track_denied=True)
    model = TopDeniedModel()
    rng = np.random.default_rng(8)
    groups = fam.groups()

    def batch(members, extra, now, what):
        keys = [k for g in groups for j, k in enumerate(g) if j % 4 in members for _ in range(3 + extra + j % 4)]
        keys = [keys[i] for i in rng.permutation(len(keys))]
        ref = apply(eng, orc, keys, SHORT, now, what=what)
        denied = (ref.allowed == 0) & (ref.status == 0)
        for k in np.array(keys, dtype=object)[denied]:
            model.update(k)
        return int(denied.sum())

    def check(what, live):
        assert eng.top_denied(10000) == model.get_top(10000), what
        assert eng.top_denied(7) == model.get_top(7), what
        assert eng.counters()["live_slots"] == live == len(orc)

    def sweep(now):
        before = len(orc)
        orc.force_cleanup(now)
        assert eng.sweep_expired(now) == before - len(orc) == before > 0

    n_all = len(fam.keys())
    assert batch({0, 1, 2, 3}, 1, T0, "first lives") > n_all         # member j of a group: 4 + j requests, burst 3 -> 1 + j denials
    g = fam.twins[0]
    assert [model.counts[k] for k in g[:4]] == [1, 2, 3, 4] and [model.counts[k] for k in fam.near["bit63"][0]] == [1, 2]
    check("bound", n_all)
    sweep(T0 + 3 * S)                                                 # every key retires with its count
    check("retired", 0)
    batch({0, 2}, 2, T0 + 4 * S, "members 0 and 2 return")            # ... and takes it back: + 2 + j
    assert [model.counts[k] for k in g[:4]] == [3, 2, 7, 4]
    check("returned", sum(1 for gr in groups for j, _ in enumerate(gr) if j % 4 in (0, 2)))
    sweep(T0 + 7 * S)
    check("retired again", 0)
    batch({1, 3}, 0, T0 + 8 * S, "members 1 and 3 return")            # + j
    assert [model.counts[k] for k in g[:4]] == [3, 3, 7, 7]
    check("second return", sum(1 for gr in groups for j, _ in enumerate(gr) if j % 4 in (1, 3)))
    sweep(T0 + 11 * S)
    check("third retirement", 0)
    assert len(model.counts) == n_all and eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    eng.close()


# ---- 8. routing with chosen owners -------------------------------------------------------------------------------------------
ROUTE_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 112, 113, 300)  # as tests/test_gpu_route_keys.py
SENT = 0x5A5A5A5A
N_ROUTE = 3000


def route_arena(world, case):
    """3 000 keys with chosen owners -> (keys, expected keys per destination)"""
    rng = np.random.default_rng(world * 10 + len(case))
    last = world - 1
    dest = {"last": [last] * N_ROUTE, "zero": [0] * (N_ROUTE - 2) + [last, 0], "alternate": [1 + j % 2 for j in range(N_ROUTE)]}[case]
    keys = []
    for j, d in enumerate(dest):
        k = ks.owned_by(d, world, rng, ROUTE_LENS[j % len(ROUTE_LENS)])
        keys.append(k if k is not None else ks.owned_by(d, world, rng, 9))  # (no 0- or 1-byte key may exist for this owner)
    want = np.bincount(dest, minlength=world)
    return keys, want


@pytest.mark.parametrize("case", ["last", "zero", "alternate"])
@pytest.mark.parametrize("world", [3, 64])
def test_route_keys_with_chosen_owners(world, case):
    import torch
    import throttlecrab_amd as t
    from oracle import oracle as O
    from throttlecrab_amd import sharded
    keys, want = route_arena(world, case)
    # as designed, before the engine is called: everything for one destination / one stray key in the last tile / destination 0 empty
    own = np.array([ks.owner(k, world) for k in keys])
    assert np.array_equal(np.bincount(own, minlength=world), want) and len({len(k) for k in keys}) >= 15
    assert {"last": want[-1] == N_ROUTE, "zero": want[0] == N_ROUTE - 1 and want[-1] == 1 and own[-2] == world - 1,
            "alternate": want[0] == 0 and want[1] == want[2] == N_ROUTE // 2 and want[3:].sum() == 0}[case]
    kb, ko = O.pack_keys(keys)
    assert np.array_equal(sharded.route_keys(kb, ko, world), own)
    n, total = len(keys), int(ko[-1])
    segs = []
    for d in range(world):  # destination d's arena by numpy indexing (as _segment of tests/test_gpu_route_keys.py)
        pos = np.nonzero(own == d)[0]
        lens = (ko[pos + 1] - ko[pos]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = np.repeat(ko[pos].astype(np.int64) - off[:-1], lens) + np.arange(off[-1])
        segs.append((off, kb[idx], pos))
    counts = np.array([len(s[2]) for s in segs] + [s[0][-1] for s in segs], dtype=np.int64)
    d_kb, d_ko = torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda()
    eng = t.Engine(1000, 1000)
    for only in sorted({-1, 0, world - 1}):
        outs = (torch.full((total + 64,), SENT & 0xFF, dtype=torch.uint8, device="cuda"), torch.full((n + world + 8,), SENT, dtype=torch.int32, device="cuda"),
                torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda"), torch.full((2 * world,), SENT, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        eng.route_keys(d_kb, d_ko, world, only=only, out=outs)
        eng.synchronize()
        ob, oo, op, oc = (x.cpu().numpy() for x in outs)
        assert np.array_equal(oc.astype(np.int64), counts), only
        k0 = b0 = 0
        for d in ([only] if only >= 0 else range(world)):
            off, byt, pos = segs[d]
            o0 = k0 + (d if only < 0 else 0)
            assert np.array_equal(oo[o0: o0 + len(pos) + 1], off), (only, d)
            assert np.array_equal(ob[b0: b0 + off[-1]], byt), (only, d)
            assert np.array_equal(op[k0: k0 + len(pos)], pos), (only, d)
            k0, b0 = k0 + len(pos), b0 + off[-1]
        assert (ob[b0:] == SENT & 0xFF).all() and (oo[k0 + (world if only < 0 else 1):] == SENT).all() and (op[k0:] == SENT).all()  # sentinels
    eng.close()
