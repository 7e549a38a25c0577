"""tc_peek_batch_keys -- the read-only resolve (hash, probe, confirm, cell, answer in one launch; nothing claimed, nothing bound) --
beside tc_throttle_batch_keys, the mutating call of the same shape, in the same process on the same engine:
    `--resident` string keys (default 10 M) bound first, then batches of `--keys` (default 1 Mi) requests of a uniform stream over
    them, device pointers, tc_throttle records out; both key sets of workload.py (`key_%d`, and 32..64 bytes of ASCII), each on an
    engine of its own; peeks at 0 % and 20 % never-seen keys, the mutating call at 0 % (it would bind the others).
Timed with events on the engine's stream: warm-up, then median and range over `--regions` regions of `--calls` calls each.
Bytes per key are counted from the shapes (what one request must touch at least), not measured.
One JSON object on stdout; --out writes it to a file as well.  Needs a GPU: there is no fallback."""
import argparse
import functools
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_PROBE_US = (68.0, 77.0)  # kt::k_probe alone inside the mutating key stage, 1 Mi lookups, 209 MB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--resident", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the result (default: git rev-parse of this tree)")
    a = ap.parse_args()
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import workload as W
    assert torch.cuda.is_available(), "peekbench needs a GPU"
    try:
        commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    res = {"tool": "peekbench", "commit": commit, "device": torch.cuda.get_device_name(0), "keys": a.keys, "resident": a.resident,
           "calls_per_region": a.calls, "regions": a.regions, "k_probe_us_design_s4": K_PROBE_US, "sets": {}}
    plan = dict(max_burst=W.REF_PARAMS[0], count_per_period=W.REF_PARAMS[1], period=W.REF_PARAMS[2], quantity=1)
    stream = torch.cuda.Stream()
    up = lambda kb, ko: (torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda())
    for name, make in (("key_%d", W.string_keys), ("ascii_32_64", W.long_keys)):
        eng = t.Engine(max(a.resident + a.resident // 10, 1 << 16), a.keys, key_mode=True)
        with torch.cuda.stream(stream):
            eng.use_torch_stream()
            for at in range(0, a.resident, a.keys):  # bind the resident keys
                eng.rate_limit_batch_keys(*up(*make(np.arange(at, min(at + a.keys, a.resident)))), now_ns=W.T0_NS, want=("allowed",), **plan)
            stream.synchronize()
            assert eng.counters()["keys_inserted"] == a.resident
            ids = W.uniform_slots(a.resident, a.keys).astype(np.int64)
            fresh = ids.copy()
            fresh[::5] += a.resident  # every fifth request: a key nobody has seen
            entry = {}
            clock = [W.T0_NS]

            def timed(call, kb, ko):
                out = None
                us = []
                for r in range(a.regions + 1):  # (region 0: warm-up -- code objects, first-touch of the outputs)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.calls):
                        clock[0] += 1_000_000
                        out = call(kb, ko, now_ns=clock[0], want=("throttle",), out=out, **plan)
                    e1.record(stream)
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
                us = us[1:]
                return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}, out

            for label, stream_ids, call in (("peek_miss_0", ids, eng.peek_batch_keys), ("peek_miss_20", fresh, eng.peek_batch_keys),
                                            ("throttle_batch_miss_0", ids, eng.rate_limit_batch_keys),
                                            ("throttle_batch_miss_0_inputs_ready", ids, functools.partial(eng.rate_limit_batch_keys, inputs_ready=True))):
                kb, ko = make(stream_ids)
                before = eng.counters()
                m, out = timed(call, *up(kb, ko))
                n, arena = len(ko) - 1, int(ko[-1])
                hit = 1.0 if stream_ids is ids else 0.8
                # per request: key bytes + two offsets, the 32-byte entry (more with collisions), for a hit on a key beyond 16 bytes its
                # 128-byte record line, the 16-byte cell of a hit, a 16-byte record out -- the mutating call moves more (slot columns,
                # grouping, the cell written back): not counted here
                m["bytes_per_key_least"] = round(arena / n + 4 + 32 + hit * ((128 if arena / n > 16 else 0) + 16) + 16, 1)
                m["ns_per_key"] = round(m["median_us"] * 1000.0 / n, 3)
                rec = eng.unpack_throttle(out.throttle)
                m["allowed_share_last_call"] = round(float(rec["allowed"].mean()), 4)
                after = eng.counters()
                m["counters_moved"] = {k: after[k] - before[k] for k in after if after[k] != before[k]}
                entry[label] = m
            entry["peek_over_throttle_batch"] = round(entry["peek_miss_0"]["median_us"] / entry["throttle_batch_miss_0"]["median_us"], 3)
        res["sets"][name] = entry
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
