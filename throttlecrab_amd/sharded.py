"""Hash-sharded multi-GPU limiter: one process per GPU, one Engine per process.

The reference has no distributed mode ("use client-side sharding by key",
README.md:247-249).  Keys are independent units, so the decision path needs NO
collective: (owner, slot) of a global key id is a bijection of the id space
(tc_route_host / rt::k_route_*); every rank decides only the requests it owns.

Two ways to bring a request to its owner:
  replicate  every rank is handed the whole global batch and keeps what it owns (tc_route_batch, only = rank):
             per-GPU routing work grows with the number of GPUs;
  exchange   every rank routes only ITS 1/N slice of the batch into one segment per destination (only = -1) and puts
             each segment into the destination's inbox (tc_forward_segments: one launch writing peer memory over
             xGMI); a destination evaluates the N inboxes of a step as ONE batch whose slot column comes in pieces
             (tc_batch.seg_slot), sources in rank order, so a key's requests keep the order of the global stream.
             Per-GPU work is independent of N.  No collective: peer copies + one mailbox word per (source,
             destination, ring slot) in shared host memory, written by the source's host once its copies have landed.
The one collective is observability: the per-GPU counter blocks (cf. throttlecrab-server/src/metrics.rs:84-94) and
the top-denied blocks are all-gathered (RCCL over xGMI on GPUs, gloo in the CPU tests).
"""
from __future__ import annotations

import numpy as np

import ctypes as C

from . import _lib as L
from . import workload as W
from ._lib import TC_CNT_COUNT, TC_CNT_NAMES


def route(global_ids: np.ndarray, world: int, keys_per_shard: int):
    """Host mirror of tc_route_batch (tc_route_host: the same bijection of [0, world * keys_per_shard) the device
    kernels use) -> (owner uint32[n], shard-local slot uint32[n]).  Needs no GPU."""
    import ctypes as C

    from . import _lib as L
    ids = np.ascontiguousarray(global_ids, dtype=np.uint32)
    owner, slot = np.empty(len(ids), np.uint32), np.empty(len(ids), np.uint32)
    rc = L.load().tc_route_host(world, keys_per_shard, len(ids), ids.ctypes.data, owner.ctypes.data, slot.ctypes.data)
    if rc != 0:
        raise ValueError(f"tc_route_host({world}, {keys_per_shard}) failed: {rc}")
    return owner, slot


def route_inverse(owner: np.ndarray, slot: np.ndarray, world: int, keys_per_shard: int) -> np.ndarray:
    """(owner, shard-local slot) -> global key id (what the all-gathered top-denied block reports)."""
    from . import _lib as L
    o, s = np.ascontiguousarray(owner, dtype=np.uint32), np.ascontiguousarray(slot, dtype=np.uint32)
    out = np.empty(len(o), np.uint64)
    rc = L.load().tc_route_inverse(world, keys_per_shard, len(o), o.ctypes.data, s.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"tc_route_inverse failed: {rc}")
    return out


def shard_requests(global_ids: np.ndarray, world: int, rank: int, keys_per_shard: int):
    """What rank `rank` keeps of a global batch: (positions in the batch, shard-local slots), in stream order --
    the host-side equivalent of tc_route_batch(only=rank)."""
    owner, slot = route(global_ids, world, keys_per_shard)
    pos = np.nonzero(owner == rank)[0]
    return pos, slot[pos]


TOPK = 100  # denied keys every rank contributes to the metrics exchange (metrics.rs:24-76: TopDeniedKeys)


def pack_top_denied(top, rank: int, world: int, keys_per_shard: int) -> np.ndarray:
    """[(slot, count)] of one shard -> int64[TOPK, 2] block of (global key id, count), zero-padded."""
    block = np.zeros((TOPK, 2), np.int64)
    if top:
        slots = np.array([s for s, _ in top[:TOPK]], np.uint32)
        block[: len(slots), 0] = route_inverse(np.full(len(slots), rank, np.uint32), slots, world, keys_per_shard).astype(np.int64)
        block[: len(slots), 1] = [c for _, c in top[:TOPK]]
    return block


def merge_top_denied(gathered: np.ndarray, k: int = TOPK):
    """all-gathered [world * TOPK, 2] blocks -> the k most denied keys of the whole system [(global id, count)]
    (a key lives on one shard, so the blocks never overlap)."""
    rows = gathered.reshape(-1, 2)
    rows = rows[rows[:, 1] > 0]
    order = np.lexsort((rows[:, 0], -rows[:, 1]))
    return [(int(rows[i, 0]), int(rows[i, 1])) for i in order[:k]]


class _DevPtrView:
    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}


def device_counter_view(engine):
    """The engine's counter block as an int64 CUDA tensor aliasing device memory
    (no host round trip before the all-gather)."""
    import torch
    return torch.as_tensor(_DevPtrView(engine.counters_device_ptr(), TC_CNT_COUNT), device=f"cuda:{engine.device}")


def all_gather_counters(local_block, dist, world: int):
    """all-gather of one counter block per rank -> (per_rank [world, 8], totals dict)."""
    import torch
    gathered = torch.zeros(world * local_block.numel(), dtype=local_block.dtype, device=local_block.device)
    dist.all_gather_into_tensor(gathered, local_block.contiguous())
    per_rank = gathered.view(world, -1)
    tot = per_rank.sum(dim=0).tolist()
    return per_rank, {k: int(tot[i]) for i, k in enumerate(TC_CNT_NAMES)}


def route_keys(key_bytes: np.ndarray, key_off: np.ndarray, world: int) -> np.ndarray:
    """Owner of every string key of an arena (tc_route_keys_host: mix64(hash(key) ^ salt) mod world) -> uint32[n].  The front
    door of a sharded key-mode deployment; needs no GPU."""
    from . import _lib as L
    kb = np.ascontiguousarray(key_bytes, dtype=np.uint8)
    ko = np.ascontiguousarray(key_off, dtype=np.uint32)
    owner = np.empty(len(ko) - 1, np.uint32)
    rc = L.load().tc_route_keys_host(world, len(ko) - 1, kb.ctypes.data, ko.ctypes.data, owner.ctypes.data)
    if rc != 0:
        raise ValueError(f"tc_route_keys_host({world}) failed: {rc}")
    return owner


def split_keys(key_bytes: np.ndarray, key_off: np.ndarray, world: int):
    """-> [(key_bytes_d, key_off_d, positions_d) for d in range(world)]: the arena cut into one arena per owner, the
    requests of an owner in stream order (so that a key's requests keep their order), + where each came from"""
    owner = route_keys(key_bytes, key_off, world)
    ko = np.asarray(key_off, dtype=np.int64)
    lens = ko[1:] - ko[:-1]
    out = []
    for d in range(world):
        pos = np.nonzero(owner == d)[0]
        off_d = np.zeros(len(pos) + 1, np.uint32)
        off_d[1:] = np.cumsum(lens[pos])
        if len(pos):
            idx = np.concatenate([np.arange(ko[p], ko[p + 1]) for p in pos]) if lens[pos].sum() else np.zeros(0, np.int64)
            bytes_d = np.asarray(key_bytes, dtype=np.uint8)[idx]
        else:
            bytes_d = np.zeros(0, np.uint8)
        if bytes_d.size == 0:
            bytes_d = np.zeros(1, np.uint8)
        out.append((bytes_d, off_d, pos))
    return out


def split_keys_device(engine, d_bytes, d_off, n: int, world: int, only: int = -1):
    """split_keys for an arena that is in device memory (tc_route_keys: CUDA uint8 bytes, int32 offsets[n + 1]), without a host
    copy of a single key.  -> ([(key_bytes_d, key_off_d, positions_d) for every destination written], counts): views into the
    router's outputs -- each a complete arena for Engine.rate_limit_batch_keys -- and the host copy of the counts
    (uint32[2 * world]: keys per destination, then bytes).  only >= 0: one entry, that destination's.  Waits for the router (the
    views' sizes are its counts)."""
    host = engine.host_alloc(2 * world + 1, np.uint32)
    host[2 * world] = 0
    obytes, ooff, pos, _ = engine.route_keys(d_bytes, d_off[: n + 1], world, only=only, host_counts=host, tag=1)
    engine.synchronize()
    assert host[2 * world] == 1
    counts = host[: 2 * world].copy()
    if only >= 0:
        c = int(counts[only])
        return [(obytes[: int(counts[world + only])], ooff[: c + 1], pos[:c])], counts
    out, k0, b0 = [], 0, 0
    for d in range(world):
        c, b = int(counts[d]), int(counts[world + d])
        out.append((obytes[b0: b0 + b], ooff[k0 + d: k0 + d + c + 1], pos[k0: k0 + c]))
        k0, b0 = k0 + c, b0 + b
    return out, counts


# ---- the exchange (see the module docstring) -------------------------------------------------------------------------
def split_segments(global_slice: np.ndarray, world: int, keys_per_shard: int):
    """Host mirror of tc_route_batch(only = -1): what one source rank sends -- [shard-local slots for destination d,
    in stream order] for d in range(world)."""
    owner, slot = route(global_slice, world, keys_per_shard)
    return [slot[owner == d] for d in range(world)]


class LocalFabric:
    """Inboxes and mailboxes of every shard in ONE process (tests: several engines on one device, where a peer copy
    degenerates to a device-to-device copy)."""

    def __init__(self, world: int, seg_cap: int, ring: int, device):
        import torch
        self.world, self.ring, self.seg_cap = world, ring, seg_cap
        self._inbox = [torch.empty((ring, world, seg_cap), dtype=torch.int32, device=device) for _ in range(world)]
        self.mail = np.zeros((world, ring, world, 2), np.uint32)  # [dst][ring slot][src] = (count, step + 1)
        self.done = np.zeros(world, np.int64)                      # [dst] steps whose inboxes may be overwritten
        self.ranks = []                                            # the ExchangeRanks driven by this one thread

    def inbox(self, dst: int, slot: int, src: int):
        return self._inbox[dst][slot, src]

    def inbox_base(self, dst: int):
        return self._inbox[dst]

    def poll(self):
        """one thread drives every shard: a rank that waits for another rank's progress has to note it itself"""
        for r in self.ranks:
            r._publish_done()

    def close(self):
        pass


class IpcFabric:
    """One process per GPU on one node: every rank allocates its inboxes in its own HBM and shares them through IPC
    memory handles (exchanged ONCE, at set-up, with all_gather_object); mailboxes live in a shared-memory segment.
    Nothing on the decision path goes through torch.distributed."""

    def __init__(self, dist, rank: int, world: int, seg_cap: int, ring: int, device):
        import torch
        from multiprocessing import shared_memory
        from torch.multiprocessing.reductions import reduce_tensor
        self.world, self.ring, self.seg_cap, self.rank = world, ring, seg_cap, rank
        mine = torch.empty((ring, world, seg_cap), dtype=torch.int32, device=device)
        handles = [None] * world
        dist.all_gather_object(handles, reduce_tensor(mine))
        self._inbox = []
        for r, (fn, args) in enumerate(handles):
            self._inbox.append(mine if r == rank else fn(*args))  # (peer access is enabled lazily by the IPC open)
        words = world * ring * world * 2
        nbytes = words * 4 + world * 8
        name = [None]
        if rank == 0:
            self._shm = shared_memory.SharedMemory(create=True, size=nbytes)
            self._shm.buf[:nbytes] = bytes(nbytes)
            name[0] = self._shm.name
        dist.broadcast_object_list(name, src=0)
        if rank != 0:
            self._shm = shared_memory.SharedMemory(name=name[0])
        self.mail = np.ndarray((world, ring, world, 2), np.uint32, buffer=self._shm.buf, offset=0)
        self.done = np.ndarray((world,), np.int64, buffer=self._shm.buf, offset=words * 4)
        dist.barrier()

    def inbox(self, dst: int, slot: int, src: int):
        return self._inbox[dst][slot, src]

    def inbox_base(self, dst: int):
        return self._inbox[dst]

    def close(self):
        self.mail = self.done = None
        try:
            self._shm.close()
            if self.rank == 0:
                self._shm.unlink()
        except (OSError, BufferError):
            pass


class ExchangeRank:
    """One rank's side of the exchange: a thin wrapper over the library's tc_exchange_* calls (csrc/exchange.hip).  Per step i
    (the caller pipelines them: route a few steps ahead of post, post ahead of the evaluation):
        route(i, slice)   this rank's slice routed straight into the destinations' inboxes (one pass, counts -> pinned memory)
        post(i)           once the router's tag is in: (count, i + 1) into every destination's mailbox
        collect(i)        every source's mailbox word of step i -> [(inbox tensor, count)]
        evaluate(i, ...)  the inboxes as ONE batch, slot column in pieces, sources in rank order
        step(i, ...)      route(i + route_ahead) + post(i + post_ahead) + evaluate(i) in ONE library call (what bench.py times)
    With a LocalFabric (several ranks driven by one thread) the library runs non-blocking and a phase whose turn has not come
    is retried after every rank has published its progress."""

    def __init__(self, engine, fabric, rank: int, world: int, slice_len: int, route_ring: int = 8):
        import ctypes as C

        from . import _lib as L
        self.eng, self.fab, self.rank, self.world = engine, fabric, rank, world
        self._lib = engine._lib
        self.route_ring = route_ring  # (kept for callers that sized buffers by it; the library keeps 8 routers' count blocks)
        self._single_thread = hasattr(fabric, "ranks")
        self._ptrs = (C.c_void_p * world)(*[fabric.inbox_base(d).data_ptr() for d in range(world)])
        cfg = L.tc_exchange_config()
        cfg.struct_size = C.sizeof(L.tc_exchange_config)
        cfg.rank, cfg.world, cfg.ring, cfg.seg_cap = rank, world, fabric.ring, fabric.seg_cap
        cfg.flags = L.TC_X_NONBLOCKING if self._single_thread else 0
        cfg.keys_per_shard = engine.capacity
        cfg.inbox = C.cast(self._ptrs, C.c_void_p)
        cfg.mail = fabric.mail.ctypes.data
        cfg.done = fabric.done.ctypes.data
        h = C.c_void_p(0)
        engine._check(self._lib.tc_exchange_create(engine._h, C.byref(cfg), C.byref(h)))
        self._h = h
        engine._children.append(self)   # (the exchange points into the engine: the engine closes it first)
        self._again = L.TC_E_AGAIN
        self._counts = (C.c_uint32 * world)()
        if self._single_thread:
            fabric.ranks.append(self)
        self.host_s = {"route": 0.0, "post": 0.0, "collect": 0.0, "evaluate": 0.0, "step": 0.0}  # host seconds per phase (diagnostics)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tc_exchange_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    RETRY_SECONDS = 60.0  # one thread driving several ranks: how long a phase is retried before the pipeline is declared stuck

    def _call(self, fn, *args):
        import time
        deadline = None
        while True:
            rc = fn(self._h, *args)
            if rc != self._again:
                self.eng._check(rc)
                return
            # TC_E_AGAIN: with TC_X_NONBLOCKING "not this phase's turn yet" -- retried, but not for ever (a mis-set pipeline, e.g.
            # post_ahead = 0 with one thread driving all ranks, never gets its turn: ADVICE r4); from a blocking exchange it
            # means the library itself gave up waiting for a peer
            if deadline is None:
                deadline = time.monotonic() + self.RETRY_SECONDS
            if not self._single_thread or time.monotonic() > deadline:
                from .engine import TcError
                raise TcError(rc, "exchange phase never got its turn (a peer rank is gone, or route_ahead / post_ahead do not fit the ring)")
            self.fab.poll()  # (one thread drives every shard: let the others publish what they have finished)

    def route(self, step: int, global_slice):
        if global_slice.numel() > self.fab.seg_cap:
            raise RuntimeError(f"a slice of {global_slice.numel()} requests exceeds the inbox capacity {self.fab.seg_cap}")
        self._keep_slice = global_slice
        self._call(self._lib.tc_exchange_route, step, global_slice.data_ptr(), global_slice.numel())

    def post(self, step: int):
        self._call(self._lib.tc_exchange_post, step)

    def collect(self, step: int):
        self._call(self._lib.tc_exchange_collect, step, self._counts)
        k = step % self.fab.ring
        return [(self.fab.inbox(self.rank, k, s), int(self._counts[s])) for s in range(self.world)]

    def _template(self, n_out, now_ns, outs, step, **kw):
        """the evaluation's tc_batch: outputs (a result set of its own per step in flight), one timestamp, the registered plans"""
        import ctypes as C
        res = outs[step % len(outs)]
        # TC_B_OUTPUTS_IDLE promises that nothing in flight touches the arrays: only with a ring longer than the pipeline
        idle = len(outs) >= 8 and kw.pop("outputs_idle", True)
        kw.pop("outputs_idle", None)
        quantity, want = kw.pop("quantity", 1), kw.pop("want", ("allowed",))
        if kw:  # (max_burst= / grouped= ... used to be dropped without a word)
            raise TypeError(f"exchange evaluation: unsupported options {sorted(kw)} (the registered plans, one timestamp, quantity, want, outputs_idle)")
        for name in want:
            # a result set may still be written by an earlier step that cycles through it: never reallocated behind its back
            cur = getattr(res, name)
            need = (n_out + 63) // 64 if name == "allowed_bits" else (4 * n_out if name in ("result4", "decisions") else n_out)
            if cur is not None and cur.numel() < need:
                raise ValueError(f"exchange evaluation: outs[{step % len(outs)}].{name} holds {cur.numel()} entries, the step may need {need} "
                                 "(it is not reallocated here: an earlier step may still be writing it)")
        b, res, keep = self.eng._prepare(n_out, True, None, None, None, quantity, now_ns, True, False, want, res, inputs_ready=True, outputs_idle=idle)
        return b, keep

    def evaluate(self, step: int, segments, now_ns: int, outs, **kw):
        """-> requests decided.  outs: a list of BatchResult to cycle through (one per step in flight).  `segments` (what
        collect() returned) only sizes the result arrays: the library reads the mailboxes itself."""
        import ctypes as C
        total = sum(cnt for _, cnt in segments) if segments is not None else self.world * self.fab.seg_cap
        if total == 0:
            total = 1  # (an empty step still has to be marked as evaluated: the library does that)
        b, keep = self._template(total, now_ns, outs, step, **kw)
        decided = C.c_uint64(0)
        self._call(self._lib.tc_exchange_evaluate, step, C.byref(b), C.byref(decided))
        self._keep_eval = keep
        return int(decided.value)

    def step(self, step: int, slice_ahead, route_ahead: int, post_ahead: int, now_ns: int, outs, **kw):
        """route(step + route_ahead, slice_ahead) + post(step + post_ahead) + evaluate(step): ONE library call.  The result arrays
        of `outs` must hold a whole step (world x seg_cap decisions at most)."""
        import ctypes as C
        b, keep = self._template(self.world * self.fab.seg_cap, now_ns, outs, step, **kw)
        decided = C.c_uint64(0)
        self._keep_slice = slice_ahead
        self._call(self._lib.tc_exchange_step, step, slice_ahead.data_ptr() if slice_ahead is not None else None,
                   slice_ahead.numel() if slice_ahead is not None else 0, route_ahead, post_ahead, C.byref(b), C.byref(decided))
        self._keep_eval = keep
        return int(decided.value)

    def timed(self, name, *args, **kw):
        """run phase `name` and book its host time (bench.py reports where a step's host time goes)"""
        import time
        t0 = time.perf_counter()
        r = getattr(self, name)(*args, **kw)
        self.host_s[name] += time.perf_counter() - t0
        return r

    def _publish_done(self):
        self._lib.tc_exchange_poll(self._h)

    def wait_us(self):
        """host microseconds spent waiting inside the library since the last call: (inbox slots, router tag, sources)"""
        import ctypes as C
        out = (C.c_uint64 * 3)()
        self._lib.tc_exchange_wait_ns(self._h, out)
        return tuple(v / 1e3 for v in out)


class ShardRank:
    """One rank's side of `replicate` mode as library calls (csrc/shard.hip: tc_shard_*): the rank is handed every global batch,
    routes it `route_ahead` steps ahead of the evaluation on the engine's grouping streams and decides what it owns -- one call
    per step (step()).  outs: a list of BatchResult to cycle through, one per step in flight, whose arrays hold the rank's
    largest share of a global batch."""

    def __init__(self, engine, rank: int, world: int, max_global: int, ring: int = 8):
        self.eng, self.rank, self.world = engine, rank, world
        self._lib = engine._lib
        cfg = L.tc_shard_config()
        cfg.struct_size = C.sizeof(L.tc_shard_config)
        cfg.rank, cfg.world, cfg.ring, cfg.keys_per_shard, cfg.max_global = rank, world, ring, engine.capacity, max_global
        h = C.c_void_p(0)
        engine._check(self._lib.tc_shard_create(engine._h, C.byref(cfg), C.byref(h)))
        self._h = h
        engine._children.append(self)   # (the shard points into the engine: the engine closes it first)
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tc_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _template(self, now_ns, outs, step, **kw):
        res = outs[step % len(outs)]
        # (round 6, late: building the tc_batch costs the host ~8 us of the ~36 a step's call takes, and between the steps of a stream
        # only the timestamp changes -- one template per result set and option set is kept; the arrays it points to are the caller's)
        ck = None
        if isinstance(now_ns, int):
            ck = (step % len(outs), id(res), tuple(sorted((k, v if isinstance(v, (int, bool, tuple, str)) else id(v)) for k, v in kw.items())),
                  tuple(id(getattr(res, f, None)) for f in ("allowed", "status", "result4", "decisions", "remaining", "limit", "reset_after_ns", "retry_after_ns", "allowed_bits")))
            hit = getattr(self, "_tmpl_cache", {}).get(ck)
            if hit is not None:
                hit[0].now_ns_scalar = now_ns
                return hit
        idle = len(outs) >= 8 and kw.pop("outputs_idle", True)
        kw.pop("outputs_idle", None)
        quantity, want = kw.pop("quantity", 1), kw.pop("want", ("allowed",))
        if kw:
            raise TypeError(f"shard evaluation: unsupported options {sorted(kw)} (the registered plans, one timestamp, quantity, want, outputs_idle)")
        n_out = min(getattr(res, name).numel() // (4 if name in ("result4", "decisions") else 1) for name in want if getattr(res, name) is not None) if any(
            getattr(res, name) is not None for name in want) else 0
        if n_out == 0:
            raise ValueError("shard evaluation: the result arrays of `outs` must be allocated by the caller (they hold a rank's largest share)")
        b, res, keep = self.eng._prepare(n_out, True, None, None, None, quantity, now_ns, True, False, want, res, inputs_ready=True, outputs_idle=idle)
        if ck is not None and isinstance(quantity, int):
            if not hasattr(self, "_tmpl_cache"):
                self._tmpl_cache = {}
            if len(self._tmpl_cache) > 256:
                self._tmpl_cache.clear()
            self._tmpl_cache[ck] = (b, keep)
        return b, keep

    def _hold_ids(self, step: int, ids):
        #  the router of `step` reads `ids` later, on one of the engine's grouping streams: a tensor the caller drops
        # must not go back to torch's allocator before that -- one reference per ring entry, as the C side keeps its columns
        if not hasattr(self, "_ids_ring"):
            self._ids_ring = {}
        self._ids_ring[step % 64] = ids

    def route(self, step: int, global_ids):
        self._hold_ids(step, global_ids)
        self.eng._check(self._lib.tc_shard_route(self._h, step, global_ids.data_ptr(), global_ids.numel()))

    def evaluate(self, step: int, now_ns: int, outs, **kw) -> int:
        b, keep = self._template(now_ns, outs, step, **kw)
        decided = C.c_uint64(0)
        self.eng._check(self._lib.tc_shard_evaluate(self._h, step, C.byref(b), C.byref(decided)))
        self._keep = keep
        return int(decided.value)

    def step(self, step: int, ids_ahead, route_ahead: int, now_ns: int, outs, **kw) -> int:
        """route(step + route_ahead, ids_ahead) + evaluate(step): ONE library call -> requests this rank decided"""
        b, keep = self._template(now_ns, outs, step, **kw)
        decided = C.c_uint64(0)
        self._hold_ids(step + route_ahead, ids_ahead)
        self.eng._check(self._lib.tc_shard_step(self._h, step, ids_ahead.data_ptr() if ids_ahead is not None else None,
                                                ids_ahead.numel() if ids_ahead is not None else 0, route_ahead, C.byref(b), C.byref(decided)))
        self._keep = keep
        return int(decided.value)

    def wait_us(self) -> float:
        out = C.c_uint64(0)
        self._lib.tc_shard_wait_ns(self._h, C.byref(out))
        return out.value / 1e3
