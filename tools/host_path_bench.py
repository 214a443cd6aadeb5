"""PCIe-inclusive throughput: frames handed over as HOST pointers (the reference's boundary: a view of the shared
FrameBuffer mmap, watsor/detection/detector.py:104-106), batch = 8, 640x480 (and 1920x1080), pageable vs page-locked.

    python tools/host_path_bench.py  [--out profiles/xxx.json] [--format rgb24,nv12,yuyv422,gray,p010le] [--size 1920x1080]

--format: the pixel format(s) the frames are handed over in (default rgb24) -- what the formats with fewer bytes per frame buy on
the PCIe-bound leg; one engine and one set of pictures per size, every format measured in the same run.  p010le (10-bit, a 16-bit
word per sample) is as many bytes as rgb24: its line shows what the conversion on the GPU costs, the gain is the host's swscale pass.
"""
import json
import os
os.environ.setdefault("WATSOR_HIP_DEV", "1")   # tools run on the development library (stage entry points, knobs, profiling)
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from watsor_amd import engine as eb                                   # noqa: E402
from oracle import yuv                                                # noqa: E402
from watsor_amd.runtime import FMT_GRAY8, FMT_NV12, FMT_P010, FMT_RGB24, FMT_YUYV422, HipEngine   # noqa: E402
from watsor_amd.synth import synthetic_frame, synthetic_weights      # noqa: E402

BATCH = 8


FORMATS = {"rgb24": FMT_RGB24, "nv12": FMT_NV12, "yuyv422": FMT_YUYV422, "gray": FMT_GRAY8, "p010le": FMT_P010}


def run(eng, frames, n_steps, fmt=FMT_RGB24):
    lanes = eng.num_slots
    ring = len(frames) // BATCH
    formats = None if fmt == FMT_RGB24 else [fmt] * BATCH
    for s in range(2 * lanes):
        eng.submit_host(s % lanes, frames[(s % ring) * BATCH:(s % ring + 1) * BATCH], formats=formats)
    eng.sync()
    t0 = time.perf_counter()
    for s in range(n_steps):
        eng.submit_host(s % lanes, frames[(s % ring) * BATCH:(s % ring + 1) * BATCH], formats=formats)
    eng.sync()
    return n_steps * BATCH / (time.perf_counter() - t0)


def as_format(rgb, name):
    """The picture as a decoder told `-pix_fmt <name>` would write it (BT.601 limited range; the 4:2:2 and gray frames are cut from
    the NV12 one: its luma, its chroma rows doubled -- the bytes that travel are what is measured, not the colours)."""
    if name == "rgb24":
        return rgb
    h, w = rgb.shape[:2]
    nv12 = yuv.yuv420_from_rgb(rgb, "nv12")
    if name == "nv12":
        return nv12
    if name == "gray":
        return nv12[:h].copy()
    if name == "p010le":   # NV12's samples as 10-bit ones (<< 2) in the high bits of a word (<< 6), handed over as the words' bytes
        return (nv12.astype(np.uint16) << 8).view(np.uint8).reshape(h * 3 // 2, w * 2)
    y = nv12[:h].reshape(h, w // 2, 2)
    uv = np.repeat(nv12[h:].reshape(h // 2, w // 2, 2), 2, axis=0)
    return np.stack([y[..., 0], uv[..., 0], y[..., 1], uv[..., 1]], axis=-1).reshape(h, w, 2)     # Y0 U Y1 V


def main():
    out = {}
    names = sys.argv[sys.argv.index("--format") + 1].lower().split(",") if "--format" in sys.argv else ["rgb24"]
    for n in names:
        if n not in FORMATS:
            sys.exit("--format %s: expected some of %s" % (n, ", ".join(FORMATS)))
    sizes = [(640, 480), (1920, 1080)]
    if "--size" in sys.argv:
        sizes = [tuple(int(x) for x in sys.argv[sys.argv.index("--size") + 1].lower().split("x"))]
    path = "/tmp/wz_hostbench/mi355x.bin"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    eb.save_engine(eb.build_engine(synthetic_weights(1234)), path)
    for (w, h) in sizes:
        eng = HipEngine(path, 0, BATCH, w, h)
        ring = 4
        pictures = [synthetic_frame(w, h, 1234 + i) for i in range(ring * BATCH)]
        for name in names:
            first = as_format(pictures[0], name)
            arena = np.empty((ring * BATCH,) + first.shape, np.uint8)   # stands in for a FrameBuffer arena
            for i in range(ring * BATCH):
                arena[i] = as_format(pictures[i], name)
            frames = [arena[i] for i in range(ring * BATCH)]
            pageable = run(eng, frames, 100, FORMATS[name])
            eng.host_register(arena)
            pinned = run(eng, frames, 200, FORMATS[name])
            eng.host_unregister(arena)
            mb = first.size / 1e6
            key = "%dx%d" % (w, h) if names == ["rgb24"] else "%dx%d %s" % (w, h, name)
            out[key] = dict(pageable_fps=round(pageable, 1), registered_fps=round(pinned, 1),
                            registered_h2d_gbs=round(pinned * mb / 1e3, 2), frame_mb=round(mb, 3))
            print("%dx%d %s: pageable %.0f frames/s, page-locked %.0f frames/s (%.1f GB/s of H2D, %.2f MB per frame)"
                  % (w, h, name, pageable, pinned, pinned * mb / 1e3, mb))
        eng.close()
    if "--out" in sys.argv:
        json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
