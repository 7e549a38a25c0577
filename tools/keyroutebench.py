"""tc_route_keys against the host path it replaces, for one key batch (default 1 Mi keys, world 8), both string key
sets of workload.py (`key_%d`, and 32..64 bytes of ASCII):
    device  Engine.route_keys on a torch stream handed to the router, timed with events on that stream: warm-up, then the median
            over `--regions` regions of `--calls` calls each; only = -1 and only = 0
    host    sharded.split_keys (tc_route_keys_host + the numpy cut), the front door a sharded key-mode deployment had before:
            median wall time over `--host-repeats` runs on the same arena
Bytes moved = arena and offsets read + arena, offsets and positions written (counted from the shapes; only = 0 writes a
world-th of them), against the 6.29 TB/s copy ceiling.  One JSON object on stdout; --out writes it to a file as well.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12  # bytes/s
KEY_STEP_US = 210.0     # a 1 Mi-key batch's step on a key-mode engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the result (default: git rev-parse of this tree)")
    a = ap.parse_args()
    import torch
    import throttlecrab_amd as t
    from throttlecrab_amd import sharded
    from throttlecrab_amd import workload as W
    assert torch.cuda.is_available(), "keyroutebench needs a GPU"
    try:
        commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    ids = W.uniform_slots(10_000_000, a.keys)
    eng = t.Engine(1000, 1000)
    stream = torch.cuda.Stream()
    res = {"tool": "keyroutebench", "commit": commit, "device": torch.cuda.get_device_name(0), "keys": a.keys, "world": a.world,
           "calls_per_region": a.calls, "regions": a.regions, "key_step_us": KEY_STEP_US, "sets": {}}
    for name, (kb, ko) in (("key_%d", W.string_keys(ids)), ("ascii_32_64", W.long_keys(ids))):
        n, arena = len(ko) - 1, int(ko[-1])
        d_kb, d_ko = torch.from_numpy(kb).cuda(), torch.from_numpy(ko.astype(np.int32)).cuda()
        entry = {"arena_bytes": arena}
        for only in (-1, 0):
            out = None
            with torch.cuda.stream(stream):
                for _ in range(5):  # warm-up: code objects, the router's scratch
                    out = eng.route_keys(d_kb, d_ko, a.world, only=only, out=out, stream=stream)
                stream.synchronize()
                us = []
                for _ in range(a.regions):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.calls):
                        eng.route_keys(d_kb, d_ko, a.world, only=only, out=out, stream=stream)
                    e1.record(stream)
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
            counts = out[3].cpu().numpy().astype(np.int64)
            kept_k = n if only < 0 else int(counts[only])
            kept_b = arena if only < 0 else int(counts[a.world + only])
            # read: arena + offsets (the count kernel), arena + offsets + owner column (the scatter); written: owner column,
            # kept bytes, offsets and positions
            moved = 2 * (arena + 4 * (n + 1)) + 2 * n + kept_b + 4 * (kept_k + (a.world if only < 0 else 1)) + 4 * kept_k
            med = statistics.median(us)
            entry["device_only_%d" % only] = {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                                             "bytes_moved": moved, "share_of_copy_ceiling": round(moved / (med * 1e-6) / COPY_CEILING, 4),
                                             "share_of_key_step": round(med / KEY_STEP_US, 3)}
        hs = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            sharded.split_keys(kb, ko, a.world)
            hs.append((time.perf_counter() - t0) * 1e6)
        hmed = statistics.median(hs)
        entry["host_split_keys"] = {"median_us": round(hmed, 1), "min_us": round(min(hs), 1), "max_us": round(max(hs), 1),
                                    "key_steps": round(hmed / KEY_STEP_US, 1),
                                    "times_device_only_-1": round(hmed / entry["device_only_-1"]["median_us"], 1)}
        res["sets"][name] = entry
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
