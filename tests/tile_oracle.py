"""CPU restatement of the tiled-detection merge (include/watsor_hip.h: wz_detect_tiled; csrc/k_tiles.hip: wz_k_merge_tiles), bit-equal
to the kernel: plain Python integers and one IEEE double division per test.

    merge_tiles(tiles, tile_rows, iou, ios) -> ROW_DTYPE[100]

tiles = [(x0, y0, w, h), ...], tile_rows = ROW_DTYPE [len(tiles), 100] in tile pixel coordinates.  The camera filter is not part of it:
the engine applies it to the 100 merged rows exactly as `HipEngine.filter_rows` does.
"""
import numpy as np

from watsor_amd.runtime import ROW_DTYPE

MAX_DETECTIONS = 100


def _i32(v: int) -> int:
    """two's complement wrap of a Python integer to int32 (the kernel adds the origin in 32 bits, nothing is clamped)"""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def _area(b) -> int:
    return (b[2] - b[0]) * (b[3] - b[1])


def boxes_match(a, b, iou: float, ios: float) -> bool:
    """a, b = (x_min, y_min, x_max, y_max).  Intersection over union above `iou`, or intersection over the smaller box above `ios`;
    a threshold >= 1 switches its test off."""
    a1, a2 = _area(a), _area(b)
    ix = max(0, min(a[2], b[2]) - max(a[0], b[0]))
    iy = max(0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = ix * iy
    uni = a1 + a2 - inter
    amin = min(a1, a2)
    if iou < 1.0 and uni > 0 and float(inter) / float(uni) > iou:
        return True
    return bool(ios < 1.0 and amin > 0 and float(inter) / float(amin) > ios)


def padding_row():
    row = np.zeros((), ROW_DTYPE)
    row["label"] = 1
    return row


def merge_tiles(tiles, tile_rows, iou: float, ios: float) -> np.ndarray:
    tile_rows = np.asarray(tile_rows, ROW_DTYPE).reshape(len(tiles), MAX_DETECTIONS)
    iou, ios = float(iou), float(ios)
    cands = []
    for t, (x0, y0, _w, _h) in enumerate(tiles):
        for r in range(MAX_DETECTIONS):
            row = tile_rows[t, r]
            label, conf = int(row["label"]), float(row["confidence"])
            if label > 0 and conf > 0.0:                       # (NaN compares false)
                box = (_i32(int(row["x_min"]) + x0), _i32(int(row["y_min"]) + y0), _i32(int(row["x_max"]) + x0), _i32(int(row["y_max"]) + y0))
                cands.append((-conf, t, r, label, box))
    cands.sort(key=lambda c: c[:3])                            # confidence descending, then tile, then row
    kept, by_label = [], {}
    for neg, _t, _r, label, box in cands:
        if len(kept) == MAX_DETECTIONS:
            break
        if any(boxes_match(k, box, iou, ios) for k in by_label.get(label, ())):
            continue
        kept.append((label, -neg, box))
        by_label.setdefault(label, []).append(box)
    out = np.zeros(MAX_DETECTIONS, ROW_DTYPE)
    out[:] = padding_row()
    for i, (label, conf, box) in enumerate(kept):
        out[i]["label"] = label
        out[i]["confidence"] = conf
        out[i]["x_min"], out[i]["y_min"], out[i]["x_max"], out[i]["y_max"] = box
    return out


def crop(frame, w: int, h: int, fmt: int, rect) -> np.ndarray:
    """The bytes of rectangle (x0, y0, tw, th) of a w x h frame of base format `fmt` (0 RGB24, 1 NV12, 2 I420, 3 YUYV422, 4 UYVY422,
    5 GRAY8, 6 BGR24) as one flat uint8 array: `np.ascontiguousarray` of the slices of every plane, one plane after the other."""
    x0, y0, tw, th = rect
    buf = np.asarray(frame, np.uint8).reshape(-1)
    base = fmt & 0xFF
    cut = lambda plane, px, py, pw, ph: np.ascontiguousarray(plane[py:py + ph, px:px + pw]).reshape(-1)      # noqa: E731
    if base in (1, 2):
        luma, chroma = buf[:w * h].reshape(h, w), buf[w * h:]
        if base == 1:
            return np.concatenate([cut(luma, x0, y0, tw, th), cut(chroma.reshape(h // 2, w), x0, y0 // 2, tw, th // 2)])
        q = (w // 2) * (h // 2)
        u, v = chroma[:q].reshape(h // 2, w // 2), chroma[q:].reshape(h // 2, w // 2)
        return np.concatenate([cut(luma, x0, y0, tw, th), cut(u, x0 // 2, y0 // 2, tw // 2, th // 2), cut(v, x0 // 2, y0 // 2, tw // 2, th // 2)])
    bpp = {0: 3, 6: 3, 3: 2, 4: 2, 5: 1}[base]
    return cut(buf.reshape(h, w, bpp), x0, y0, tw, th)


def tile_shape(tw: int, th: int, fmt: int):
    """The array shape `HipEngine.frame_geometry` expects for a tw x th frame of base format `fmt`."""
    base = fmt & 0xFF
    return {0: (th, tw, 3), 6: (th, tw, 3), 1: (th * 3 // 2, tw), 2: (th * 3 // 2, tw), 3: (th, tw, 2), 4: (th, tw, 2), 5: (th, tw)}[base]
