#!/usr/bin/env python3
"""Colour-file throughput: single 8192^2 encodes (jpegamd_encode_color_async) at 4:2:0 and 4:4:4, timed through the profiling
ring (every kernel's own begin / end events), with the per-kernel durations.  Prints one JSON line per subsampling.

  python tools/bench_color.py [--size 8192] [--steps 50] [--warmup 10] [--quality 50] [--kind 0]

With --batch N the same timed loop goes through jpegamd_encode_color_batch_async: N distinct pictures (seeds 1 .. N) per call,
reported as the whole call's time (ns_total) per picture, and Gpixels/s.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "jpeg-image-compression_amd" / "python"))

KERNELS = ["k_chroma_planes", "Y k_tile_encode", "Y k_segment_merge", "Y k_finalize", "Cb k_tile_encode", "Cb k_segment_merge",
           "Cb k_finalize", "Cr k_tile_encode", "Cr k_segment_merge", "Cr k_finalize", "k_append_scans"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--batch", type=int, default=None, help="pictures per call through the colour batch entry (1 .. 32)")
    a = ap.parse_args()
    import torch                          # (the device runtime comes up through torch first, as in bench.py)
    if not torch.cuda.is_available():
        sys.exit("bench_color.py: no GPU")
    torch.cuda.set_device(0)
    import jpegamd

    dev = torch.device("cuda:0")
    w = h = a.size
    if a.batch is not None:
        run_batch(a, jpegamd, torch, dev)
        return
    bmp = jpegamd.synth_bmp(w, h, 1, a.kind, 0)
    img, off = jpegamd.parse_bmp(bmp)
    px = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev)
    desc = jpegamd.Encoder.image(px.data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality)
    enc = jpegamd.Encoder(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    for sub, name in ((jpegamd.SUBSAMPLE_420, "420"), (jpegamd.SUBSAMPLE_444, "444")):
        cap = jpegamd.max_jfif_bytes_color(w, h, sub)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(a.warmup):
            enc.encode_color_async(desc, sub, out.data_ptr(), cap, size.data_ptr(), stream)
        enc.finish()
        enc.set_profiling(a.steps)
        for _ in range(a.steps):
            enc.encode_color_async(desc, sub, out.data_ptr(), cap, size.data_ptr(), stream)
        st = enc.finish()
        per = [enc.color_profile(i) for i in range(a.steps)]
        totals = [enc.profile(i).ns_total for i in range(a.steps)]
        enc.set_profiling(0)
        med = {k: int(statistics.median(p[i] for p in per)) for i, k in enumerate(KERNELS)}
        t = statistics.median(totals)
        print(json.dumps({"subsampling": name, "width": w, "height": h, "quality": a.quality, "kind": a.kind, "steps": a.steps,
                          "bytes": int(size.item()), "entropy_bits": st.entropy_bits, "ns_total_median": int(t),
                          "gpixels_per_s": round(w * h / t, 2), "kernel_ns_median": med,
                          "kernel_ns_sum": sum(med.values())}))


def run_batch(a, jpegamd, torch, dev) -> None:
    w = h = a.size
    n = a.batch
    pxs, descs = [], []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        pxs.append(torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev))
        descs.append(jpegamd.Encoder.image(pxs[-1].data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality))
        del bmp
    enc = jpegamd.Encoder(w, n * h)
    stream = torch.cuda.current_stream().cuda_stream
    for sub, name in ((jpegamd.SUBSAMPLE_420, "420"), (jpegamd.SUBSAMPLE_444, "444")):
        cap = jpegamd.max_jfif_bytes_color(w, h, sub)
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        out_ptrs = [o.data_ptr() for o in outs]
        size_ptrs = [sizes.data_ptr() + 8 * i for i in range(n)]
        for _ in range(a.warmup):
            enc.encode_color_batch_async(descs, sub, out_ptrs, cap, size_ptrs, stream)
        enc.finish()
        enc.set_profiling(a.steps)
        for _ in range(a.steps):
            enc.encode_color_batch_async(descs, sub, out_ptrs, cap, size_ptrs, stream)
        st = enc.finish()
        totals = [enc.profile(i).ns_total for i in range(a.steps)]
        enc.set_profiling(0)
        t = statistics.median(totals)
        print(json.dumps({"subsampling": name, "width": w, "height": h, "batch": n, "quality": a.quality, "kind": a.kind,
                          "steps": a.steps, "bytes": sizes.cpu().tolist(), "entropy_bits": st.entropy_bits,
                          "ns_total_median": int(t), "us_per_picture": round(t / n / 1000, 1),
                          "gpixels_per_s": round(n * w * h / t, 2)}))
        del outs


if __name__ == "__main__":
    main()
