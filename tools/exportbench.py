"""tc_export_live -- one whole-capacity export of a key-mode engine (`--resident` bound `key_%d` keys, default 10 M) -- beside the
key sweep's scan over the same table (tc_sweep_expired at a time at which nothing has expired: the same `bound` bytes and cells
are read, nothing is freed), and tc_import_live of the first `--keys` (default 1 Mi) exported entries into a fresh engine: the
first call binds them (the insert stage + the merge), the repeats find them.
Timed with events on the engine's stream: a warm-up region, then median and range over `--regions` regions of `--calls` calls.
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import workload as W
    assert torch.cuda.is_available(), "exportbench needs a GPU"
    plan = dict(max_burst=W.REF_PARAMS[0], count_per_period=W.REF_PARAMS[1], period=W.REF_PARAMS[2], quantity=1)
    cap = max(a.resident + a.resident // 10, 1 << 16)
    res = {"tool": "exportbench", "device": torch.cuda.get_device_name(0), "resident": a.resident, "capacity": cap, "import_entries": a.keys,
           "calls_per_region": a.calls, "regions": a.regions}
    stream = torch.cuda.Stream()
    eng, dst = t.Engine(cap, a.keys, key_mode=True), t.Engine(2 * a.keys, a.keys, key_mode=True)
    with torch.cuda.stream(stream):
        eng.use_torch_stream()
        dst.use_torch_stream()
        for at in range(0, a.resident, a.keys):  # bind the resident keys
            kb, ko = W.string_keys(np.arange(at, min(at + a.keys, a.resident)))
            eng.rate_limit_batch_keys(torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda(), now_ns=W.T0_NS, want=("allowed",), **plan)
        stream.synchronize()
        assert eng.counters()["keys_inserted"] == a.resident
        out = eng.export_buffers(a.resident, 24 * a.resident)

        def timed(call, regions=a.regions, calls=a.calls):
            us = []
            for _ in range(regions + 1):  # (region 0: warm-up -- code objects, first touch of the outputs)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    call()
                e1.record(stream)
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1000.0 / calls)
            us = us[1:]
            return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}

        res["export_whole_capacity"] = timed(lambda: eng.export_live(out, W.T0_NS + 1))
        entries, nbytes = (int(v) for v in out["count"].tolist())
        assert entries == a.resident
        # what the three launches must move at least: `bound` and cells twice, a record line per live key twice, the outputs once
        res["export_whole_capacity"].update(entries=entries, key_bytes=nbytes, bytes_least=2 * (cap * 17 + entries * 128) + entries * 24 + nbytes)
        res["key_sweep_nothing_expired"] = timed(lambda: eng.sweep_expired_async(W.T0_NS + 1))
        assert eng.counters()["swept"] == 0
        n = min(a.keys, entries)
        imp = lambda: dst.import_live(n, out["tat"], out["expiry"], key_bytes=out["key_bytes"], key_off=out["key_off"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        cnt = imp()
        e1.record(stream)
        e1.synchronize()
        assert cnt.tolist() == [n, 0]
        res["import_first_call_binds"] = {"us": round(e0.elapsed_time(e1) * 1000.0, 1), "entries": n}
        res["import_repeat_finds"] = timed(imp)
    eng.close()
    dst.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
