#!/usr/bin/env python3
"""The image import kernel (k_import_image) per layout, next to the frame
import (k_import_rgb8 on RGBA) as the yardstick, and what the in-place read
saves a caller who holds a float CHW tensor.

  python tools/import_bench.py [--out FILE] [--batches 8] [--per-batch 25] [--encodes 9]     (GPU box)

Sizes 1920x1080 and 3840x2160; layouts CHW u8, CHW f32, HWC BGR u8, HW u8,
all resident in HBM.  Per layout, after a warm-up, `batches` batches of
`per-batch` imports (gz.image_pack) alternate one by one with the yardstick
(gz.frame_pack of an RGBA frame of the same size) in one process.  Kernel
time is the library's own per-launch HIP-event timing (gz.profile_read:
ref_import_image, ref_import); a layout's figure is the median of its batch
means, min and max beside it.  Bytes per pixel are computed from the shape:
the samples read plus the 3 bytes of P and the 12 bytes of the linear planes
written.  Then, at 1080p q95, the medians over `encodes` encodes (after one
warm-up) of process_image's seconds_setup on a planar float tensor, and of
the torch conversion to contiguous HWC u8 plus process_frame's seconds_setup;
the two ways must encode the same bytes.  Writes one JSON document to stdout
and to FILE (default profiles/image_import.json) and prints the table for
DESIGN §13."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guetzli-cuda-opencl_amd", "python"))
import guetzli_amd as gz  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]
WRITTEN = 3 + 12  # P and the three linear planes, bytes per pixel
# label: (channels read, bytes per sample, keyword arguments)
LAYOUTS = {"chw_u8": (3, 1, {}), "chw_f32": (3, 4, {}), "hwc_bgr_u8": (3, 1, {"order": "BGR"}), "hw_u8": (1, 1, {})}
YARDSTICK_BYTES = 4 + WRITTEN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_import.json"))
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--per-batch", type=int, default=25)
    ap.add_argument("--encodes", type=int, default=9)
    args = ap.parse_args()
    import numpy as np
    import torch

    torch.ones(1, device="cuda:0").item()  # torch's HIP runtime before the library's
    if gz.device_count() == 0:
        sys.exit("import_bench: no HIP device")
    doc = {"imports_per_layout": args.batches * args.per_batch, "written_bytes_per_pixel": WRITTEN, "sizes": []}

    def batch_means(t, kw, rgba):
        """Per batch the mean kernel time (us) of the layout and of the yardstick."""
        mine, yard = [], []
        for _ in range(args.batches):
            gz.profile_reset()
            for _ in range(args.per_batch):
                gz.frame_pack(rgba)
                gz.image_pack(t, **kw)
            prof = gz.profile_read()
            (c0, ms0), (c1, ms1) = prof["ref_import"], prof["ref_import_image"]
            assert c0 == c1 == args.per_batch, (c0, c1)
            yard.append(1e3 * ms0 / c0)
            mine.append(1e3 * ms1 / c1)
        return mine, yard

    def figure(us, bytes_per_pixel, n):
        med = statistics.median(us)
        return {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                "bytes_per_pixel": bytes_per_pixel, "gb_per_s": round(bytes_per_pixel * n / med / 1e3, 1)}

    for w, h in SIZES:
        host = gz.synthetic_frame(0, w, h).reshape(h, w, 3)
        rgb = torch.from_numpy(host).to("cuda:0")
        rgba = torch.cat([rgb, torch.full((h, w, 1), 255, dtype=torch.uint8, device="cuda:0")], dim=2).contiguous()
        chw = rgb.permute(2, 0, 1).contiguous()
        tensors = {"chw_u8": chw, "chw_f32": chw.to(torch.float32) / 255.0,
                   "hwc_bgr_u8": rgb.flip(2).contiguous(), "hw_u8": chw[1].contiguous()}
        torch.cuda.synchronize()
        # every layout imports what it should, before anything is timed
        for label, t in tensors.items():
            want = np.repeat(host[..., 1:2], 3, axis=2) if label == "hw_u8" else host
            if not np.array_equal(gz.image_pack(t, **LAYOUTS[label][2]), want):
                sys.exit("import_bench: %s imports a wrong image" % label)
        if not np.array_equal(gz.frame_pack(rgba), host):
            sys.exit("import_bench: the yardstick imports a wrong image")
        gz.profile_enable(True)
        rec = {"w": w, "h": h, "layouts": {}}
        for label, t in tensors.items():
            channels, sample_bytes, kw = LAYOUTS[label]
            mine, yard = batch_means(t, kw, rgba)
            m = figure(mine, channels * sample_bytes + WRITTEN, w * h)
            y = figure(yard, YARDSTICK_BYTES, w * h)
            m["yardstick"] = y
            m["gb_per_s_ratio_to_yardstick"] = round(m["gb_per_s"] / y["gb_per_s"], 3)
            rec["layouts"][label] = m
        gz.profile_enable(False)
        doc["sizes"].append(rec)

    # what a caller with a float CHW tensor does today, next to the in-place read (1080p)
    w, h = SIZES[0]
    p = gz.Params.for_quality(95)
    f32 = torch.from_numpy(gz.synthetic_frame(0, w, h).reshape(h, w, 3)).to("cuda:0").permute(
        2, 0, 1).contiguous().to(torch.float32) / 255.0  # planar, as a model's output is
    torch.cuda.synchronize()
    setup_image, convert, setup_frame = [], [], []
    for rep in range(args.encodes + 1):
        data_a, st_a = gz.process_image(f32, p, return_stats=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u8 = (f32.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        data_b, st_b = gz.process_frame(u8, p, return_stats=True)
        if data_a != data_b:
            sys.exit("import_bench: the two ways encode different bytes")
        if rep:  # (the first pass warms both ways up)
            setup_image.append(st_a.seconds_setup)
            convert.append(dt)
            setup_frame.append(st_b.seconds_setup)
    doc["caller_today_1080p"] = {
        "w": w, "h": h, "encodes": args.encodes, "figures": "medians",
        "process_image_chw_f32_seconds_setup": round(statistics.median(setup_image), 6),
        "torch_convert_to_hwc_u8_seconds": round(statistics.median(convert), 6),
        "process_frame_seconds_setup": round(statistics.median(setup_frame), 6)}

    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("\n| size | layout | us (min-max) | B/px | GB/s | yardstick us | yardstick GB/s | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for rec in doc["sizes"]:
        for label, m in rec["layouts"].items():
            y = m["yardstick"]
            print("| %dx%d | %s | %.1f (%.1f-%.1f) | %d | %.0f | %.1f | %.0f | %.2f |" % (
                rec["w"], rec["h"], label, m["us"], m["us_min"], m["us_max"], m["bytes_per_pixel"], m["gb_per_s"],
                y["us"], y["gb_per_s"], m["gb_per_s_ratio_to_yardstick"]))


if __name__ == "__main__":
    main()
