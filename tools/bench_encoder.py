#!/usr/bin/env python3
"""The frame queue (guetzli_amd.Encoder) next to the hand-rolled one it
replaces, and the device import of a padded RGBA frame next to the tight
path's copy + linear pass.

  python tools/bench_encoder.py [--out FILE] [--rounds 3] [--steps 20] [--in-flight 8]     (GPU box)

Workload: 1080p q95, synthetic seeds 0-7 resident in HBM, `steps` rounds of
the eight frames per leg, after a warm-up step.  The legs alternate in one
process:
  A  a ThreadPoolExecutor over process_device (bench.py's method)
  B  Encoder.map
Every output is checked against tests/golden/manifest.json.  Writes JSON
lines (each leg, the medians, the import figures) to stdout and to FILE
(default profiles/encoder_queue_1080p.jsonl)."""
import argparse
import concurrent.futures
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guetzli-cuda-opencl_amd", "python"))
import guetzli_amd as gz  # noqa: E402

W, H, Q = 1920, 1080, 95


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_queue_1080p.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--in-flight", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    import torch

    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["synthetic"]
    want = [manifest["synth_%dx%d_s%d_q%d" % (W, H, s, Q)]["sha256"] for s in range(8)]
    params = gz.Params.for_quality(Q)
    torch.ones(1, device="cuda:0").item()  # torch's HIP runtime before the library's
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as gen:
        host = list(gen.map(lambda s: gz.synthetic_frame(s, W, H), range(8)))
    frames = [torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    order = [f for _ in range(args.steps) for f in range(8)]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def check(outs, idx):
        bad = [i for i, b in zip(idx, outs) if hashlib.sha256(b).hexdigest() != want[i]]
        if bad:
            sys.exit("bench_encoder: outputs differ from the reference for seeds %s" % sorted(set(bad)))

    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.in_flight)
    enc = gz.Encoder(device=0, in_flight=args.in_flight)

    def leg_a(idx):
        return list(pool.map(lambda i: gz.process_device(frames[i].data_ptr(), W, H, params), idx))

    def leg_b(idx):
        return list(enc.map((frames[i] for i in idx), params))

    legs = (("A", "ThreadPoolExecutor + process_device", leg_a), ("B", "Encoder.map", leg_b))
    for _, _, fn in legs:  # warm-up: engines of this size pooled, code paths touched
        check(fn(list(range(8))), list(range(8)))
    rates = {"A": [], "B": []}
    for rnd in range(args.rounds):
        for name, what, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = fn(order)
            dt = time.perf_counter() - t0
            check(outs, order)
            rates[name].append(len(order) * W * H / dt / 1e6)
            emit({"leg": name, "method": what, "round": rnd, "frames": len(order), "in_flight": args.in_flight,
                  "seconds": round(dt, 4), "mp_per_s": round(rates[name][-1], 2), "outputs_ok": len(outs)})
    # where B's frames wait, should the legs differ: per-job queueing and encode times
    jobs = [enc.submit(frames[i], params) for i in order[:32]]
    stats = [j.result(return_stats=True)[1] for j in jobs]
    med = {k: statistics.median(v) for k, v in rates.items()}
    emit({"summary": "queue", "median_mp_per_s": {k: round(v, 2) for k, v in med.items()},
          "b_over_a": round(med["B"] / med["A"], 4), "rounds": args.rounds,
          "b_seconds_queued_median": round(statistics.median(j.seconds_queued for j in jobs), 4),
          "b_seconds_total_median": round(statistics.median(s.seconds_total for s in stats), 4)})
    enc.close()
    pool.shutdown()

    # ---- the import kernel (per-launch HIP events; one frame at a time) ----
    rgba = np.full((H, W, 4), 255, np.uint8)
    rgba[..., :3] = host[0]
    forms = {}
    for label, pad, off in (("rgba_aligned", 64, 0), ("rgba_unaligned", 3, 1)):
        stride = 4 * W + pad
        buf = torch.zeros(off + stride * H, dtype=torch.uint8, device="cuda:0")
        v = buf[off:].as_strided((H, W, 4), (stride, 4, 1))
        v.copy_(torch.from_numpy(rgba).to("cuda:0"))
        forms[label] = v
    forms["rgb_tight"] = frames[0]
    torch.cuda.synchronize()
    gz.profile_enable(True)
    reps = 5
    rec = {"summary": "import", "w": W, "h": H, "reps": reps}
    for label, t in forms.items():
        gz.profile_reset()
        for _ in range(reps):
            check([gz.process_frame(t, params)], [0])
        prof = gz.profile_read()
        for region in ("ref_import", "ref_linear"):
            if region in prof:
                c, ms = prof[region]
                rec["%s_%s_us" % (label, region)] = round(1e3 * ms / c, 2)
    gz.profile_enable(False)
    # the tight path's device-to-device copy of the frame, timed the same way
    dst = torch.empty_like(frames[0])
    times = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(frames[0])
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    rec["rgb_tight_copy_us"] = round(1e3 * statistics.median(times), 2)
    emit(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
