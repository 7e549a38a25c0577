"""tc_forget_batch -- named keys out of a live engine (probe + cell gather in one launch, the removal in a second) -- beside
tc_peek_batch_keys, which performs the same probe and cell gather read-only, in the same process on the same engine:
    `--resident` string keys `key_%d` (default 10 M) bound first; a batch of `--keys` (default 1 Mi) requests of a uniform stream
    over them (duplicates included, as the peek's), device pointers.
A forget cannot be repeated on the same keys (the second call finds none of them), so a region is ONE call between two events on
the engine's stream, and the keys are bound again, untimed, before the next region; `forget_unknown` is the call once more on the
keys it has just removed (every probe ends at an empty entry, nothing is removed).  The peek is timed as tools/peekbench.py times
it: `--calls` calls per region.  Warm-up region first, then median and range over `--regions` regions.
One JSON object on stdout; --out writes it to a file as well.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--resident", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import workload as W
    assert torch.cuda.is_available(), "forgetbench needs a GPU"
    plan = dict(max_burst=W.REF_PARAMS[0], count_per_period=W.REF_PARAMS[1], period=W.REF_PARAMS[2], quantity=1)
    stream = torch.cuda.Stream()
    up = lambda kb, ko: (torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda())
    summary = lambda us: {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
    eng = t.Engine(max(a.resident + a.resident // 10, 1 << 16), a.keys, key_mode=True)
    with torch.cuda.stream(stream):
        eng.use_torch_stream()
        for at in range(0, a.resident, a.keys):  # bind the resident keys
            eng.rate_limit_batch_keys(*up(*W.string_keys(np.arange(at, min(at + a.keys, a.resident)))), now_ns=W.T0_NS, want=("allowed",), **plan)
        stream.synchronize()
        assert eng.counters()["keys_inserted"] == a.resident
        ids = W.uniform_slots(a.resident, a.keys).astype(np.int64)
        distinct = int(np.unique(ids).size)
        kb, ko = up(*W.string_keys(ids))
        live = torch.empty(a.keys, dtype=torch.uint8, device="cuda")
        cnt = torch.empty(2, dtype=torch.int64, device="cuda")

        def region(call, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / calls

        out = [None]

        def peek():
            out[0] = eng.peek_batch_keys(kb, ko, now_ns=W.T0_NS + 1, want=("throttle",), out=out[0], **plan)

        forget = lambda: eng.forget_batch(a.keys, W.T0_NS + 1, key_bytes=kb, key_off=ko, was_live=live, out_count=cnt)
        us = {"peek": [], "forget": [], "forget_unknown": []}
        for r in range(a.regions + 1):  # (region 0: warm-up -- code objects, first touch of the outputs)
            us["peek"].append(region(peek, a.calls))
            us["forget"].append(region(forget, 1))
            assert cnt.tolist() == [distinct, distinct] and int(live.sum()) == a.keys, "every named key was resident and live"
            us["forget_unknown"].append(region(forget, 1))
            assert cnt.tolist() == [0, 0] and int(live.sum()) == 0
            eng.rate_limit_batch_keys(kb, ko, now_ns=W.T0_NS, want=("allowed",), **plan)  # bound again: the next region finds them
            stream.synchronize()
        assert eng.debug_check_keys() == 0 and eng.selfcheck() == 0
    res = {"tool": "forgetbench", "device": torch.cuda.get_device_name(0), "keys": a.keys, "distinct_keys": distinct, "resident": a.resident,
           "regions": a.regions, "peek_calls_per_region": a.calls, **{k: summary(v[1:]) for k, v in us.items()}}
    res["forget_over_peek"] = round(res["forget"]["median_us"] / res["peek"]["median_us"], 3)
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
