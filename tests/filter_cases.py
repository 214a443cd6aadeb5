"""Known-answer cases for the per-camera filters (`wz_apply_filter`, `wz_k_filter_rows`, `wz_k_sat_rows`, `wz_k_sat_cols` in
csrc/k_post.hip) and a numpy reference of the lattice rule.  No GPU here: tests/test_filter_cases_cpu.py proves the builders and the
reference, tests/test_gpu_filter_edges.py runs the cases on the engine.

Two references:
  * the LITERAL one -- `oracle.filters.{Confidence,Area,Mask}Filter` on `Detection` records, zones as contour polygons
    (`literal_verdict`) -- wherever a mask goes through `HipCameraFilter`;
  * `lattice_verdict` -- clamp the box to the frame, then ask a summed-area table of the zone's filled lattice points -- wherever raw
    fill planes go through `HipEngine.set_camera_filter`.  It works on Python integers; `defect=` swaps in one seeded mistake at a
    time, which is how the cases prove that they can see it.
"""
import functools

import numpy as np

from oracle import filters as of
from oracle import zones as oz
from watsor_amd.coco import COCO_CLASSES
from watsor_amd.runtime import ROW_DTYPE
from watsor_amd.share import BoundingBox, Detection

NUM_LABELS = len(COCO_CLASSES)        # WZ_NUM_LABELS
ROW_ZONES = 10                        # WZ_MAX_ZONES: zones a row reports
CAM_ZONES = 40                        # WZ_MAX_ZONES_PER_CAM
CALL_ROWS = 100                       # rows of one filter_rows call
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DEFECTS = ("lookup", "row0", "noclamp", "cap9", "gt", "extent32")


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def make_rows(dets):
    """[(label, confidence, (x_min, y_min, x_max, y_max)), ...] -> ROW_DTYPE rows, zones and _pad zero."""
    rows = np.zeros(len(dets), ROW_DTYPE)
    for i, (label, conf, box) in enumerate(dets):
        rows[i]["label"], rows[i]["confidence"] = label, conf
        rows[i]["x_min"], rows[i]["y_min"], rows[i]["x_max"], rows[i]["y_max"] = box
    return rows


def calls(rows):
    """The rows as `filter_rows` takes them: (start, 100 rows) per call, the last call padded with all-zero rows."""
    for start in range(0, len(rows), CALL_ROWS):
        chunk = np.zeros(CALL_ROWS, ROW_DTYPE)
        part = rows[start:start + CALL_ROWS]
        chunk[:len(part)] = part
        yield start, chunk


def f32(v):
    """A score as the detector hands it over: a float32 widened to double."""
    return float(np.float32(v))


# ---- the literal reference ----------------------------------------------------------------------------------------------------
def literal_filters(cfg, alpha=None):
    filters = [of.ConfidenceFilter(cfg), of.AreaFilter(cfg)]
    if alpha is not None:
        filters.append(of.MaskFilter(cfg, alpha=alpha))
    return filters


def literal_verdict(filters, rows):
    """`label > 0 and all(f(d) for f in filters)` per row on Python integers (track.py:26): (pass[n], zones[n, 10])."""
    n = len(rows)
    out_pass, zones = np.zeros(n, np.uint8), np.zeros((n, ROW_ZONES), np.int32)
    for i in range(n):
        r = rows[i]
        d = Detection(label=int(r["label"]), confidence=float(r["confidence"]),
                      bounding_box=BoundingBox(int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])))
        out_pass[i] = 1 if (d.label > 0 and all(f(d) for f in filters)) else 0
        zones[i] = list(d.zones)
    return out_pass, zones


# ---- the lattice reference ----------------------------------------------------------------------------------------------------
class Camera:
    """What `set_camera_filter` takes: thresholds per label (NaN = not configured), fill planes [nz, H, W] (None = no mask, nz == 0 = a
    mask without zones) and the allow table [labels, nz] (None = every zone for every label)."""

    def __init__(self, width, height, conf, area, fill=None, allow=None):
        self.width, self.height = int(width), int(height)
        self.conf, self.area = np.asarray(conf, np.float64), np.asarray(area, np.float64)
        self.fill = None if fill is None else np.asarray(fill, np.uint8).reshape(-1, self.height, self.width)
        self.allow = None if allow is None else np.asarray(allow, np.uint8)
        self._tables = {}

    @classmethod
    def plain(cls, width, height, fill=None, allow=None, conf=0.0, area=0.0, labels=range(1, NUM_LABELS)):
        """Every label of `labels` configured with the same two thresholds."""
        c, a = np.full(NUM_LABELS, np.nan), np.full(NUM_LABELS, np.nan)
        for l in labels:
            c[l], a[l] = conf, area
        return cls(width, height, c, a, fill, allow)

    @classmethod
    def from_config(cls, cfg, alpha=None):
        """The constructors of confidence.py:10-15, area.py:10-17 and mask.py:17-42, the zones filled from the ORACLE's polygons."""
        width, height = cfg["width"], cfg["height"]
        conf, area = np.full(NUM_LABELS, np.nan), np.full(NUM_LABELS, np.nan)
        max_area = abs(((width - 1) - 0 + 1) * ((height - 1) - 0 + 1))
        for entry in cfg["detect"]:
            name = next(iter(entry))
            idx = COCO_CLASSES.index(name)
            conf[idx] = entry[name]["confidence"] / 100
            area[idx] = entry[name]["area"] / 100 * max_area
        fill = allow = None
        if alpha is not None:
            fill = oz.zone_fill(alpha)
            nz = fill.shape[0]
            allow = np.ones((NUM_LABELS, nz), np.uint8)
            for entry in cfg["detect"]:
                name = next(iter(entry))
                zones = entry[name]["zones"]
                if zones:
                    allow[COCO_CLASSES.index(name)] = [1 if z + 1 in zones else 0 for z in range(nz)]
        return cls(width, height, conf, area, fill, allow)

    def engine_args(self):
        """(width, height, conf, area, fill, allow) for `HipEngine.set_camera_filter`."""
        return self.width, self.height, self.conf, self.area, self.fill, self.allow

    def tables(self, defect=None):
        """Summed-area tables [nz, H + 1, W + 1], flattened: row 0 and column 0 are zero, entry (y + 1, x + 1) counts the non-zero
        fill bytes of [0..x] x [0..y]."""
        key = "row0" if defect == "row0" else None
        if key not in self._tables:
            nz = self.fill.shape[0]
            t = np.zeros((nz, self.height + 1, self.width + 1), np.int32)
            if nz:
                t[:, 1:, 1:] = (self.fill != 0).astype(np.int32).cumsum(1, dtype=np.int32).cumsum(2, dtype=np.int32)
            if key == "row0":                          # nobody zeroed row 0: whatever lay there (the column pass never reads it)
                t[:, 0, :] = np.arange(self.width + 1, dtype=np.int32)
            self._tables[key] = t.reshape(-1)
        return self._tables[key]


def _wrap32(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def lattice_verdict(cam, rows, defect=None):
    """(pass[n], zones[n, 10]) of `label > 0 and Confidence and Area and Mask`, short-circuit left to right, the mask by the lattice
    rule: a zone is hit iff one of its filled lattice points lies in the closed box clamped to the frame."""
    assert defect is None or defect in DEFECTS
    n = len(rows)
    out_pass, zones = np.zeros(n, np.uint8), np.zeros((n, ROW_ZONES), np.int32)
    W, H = cam.width, cam.height
    nz = 0 if cam.fill is None else cam.fill.shape[0]
    table = cam.tables(defect) if nz else None
    stride, plane = W + 1, (W + 1) * (H + 1)
    cap = ROW_ZONES - 1 if defect == "cap9" else ROW_ZONES
    reach = 0 if defect == "lookup" else 1               # the table entry of pixel (x, y) is (x + 1, y + 1)

    def at(p, y, x):
        i = p * plane + y * stride + x
        return int(table[i]) if 0 <= i < len(table) else 0   # (only `noclamp` ever leaves the table)

    def ge(a, b):
        return a > b if defect == "gt" else a >= b

    for i in range(n):
        r = rows[i]
        label, conf = int(r["label"]), float(r["confidence"])
        if not 0 < label < NUM_LABELS:
            continue
        ct, ar_thr = float(cam.conf[label]), float(cam.area[label])
        if ct != ct or not ge(conf, ct):
            continue
        x_min, y_min, x_max, y_max = int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])
        ex, ey = x_max - x_min + 1, y_max - y_min + 1
        if defect == "extent32":
            ex, ey = _wrap32(ex), _wrap32(ey)
        if ar_thr != ar_thr or not ge(abs(ex * ey), ar_thr):
            continue
        ok = True
        if cam.fill is not None:
            x0, x1, y0, y1 = min(x_min, x_max), max(x_min, x_max), min(y_min, y_max), max(y_min, y_max)
            if defect != "noclamp":
                x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
            ok, z = False, 0
            for p in range(nz):
                if z >= cap:
                    break
                if cam.allow is not None and not cam.allow[label][p]:
                    continue
                if x0 <= x1 and y0 <= y1 and \
                        at(p, y1 + reach, x1 + reach) - at(p, y0, x1 + reach) - at(p, y1 + reach, x0) + at(p, y0, x0) > 0:
                    zones[i][z] = p + 1
                    z += 1
                    ok = True
        out_pass[i] = 1 if ok else 0
    return out_pass, zones


# ---- 1. the exhaustive sweep on a tiny mask ------------------------------------------------------------------------------------
SWEEP_W, SWEEP_H = 13, 11
SWEEP_BOXES = 43460
SWEEP_ZONE_POINTS = (9, 43, 3)
SWEEP_ZONE_HITS = (11358, 30731, 7759)
SWEEP_LABELS = (1, 3, 8)


def sweep_alpha():
    """Three zones: a block in the top left corner, a ring (its hole is filled) joined diagonally to an L against the right and the
    bottom edge, three pixels in the top right corner."""
    a = np.full((SWEEP_H, SWEEP_W), 100, np.uint8)
    a[0:3, 0:3] = 255
    a[8:11, 9:13] = 255
    a[5:11, 11:13] = 255
    a[3:8, 4:9] = 255
    a[4:7, 5:8] = 0
    a[0, 11] = a[0, 12] = a[1, 11] = 255
    return a


def sweep_config():
    return {"width": SWEEP_W, "height": SWEEP_H,
            "detect": [{"person": {"area": 0, "confidence": 0, "zones": []}},
                       {"car": {"area": 0, "confidence": 0, "zones": [2]}},
                       {"truck": {"area": 0, "confidence": 0, "zones": [1, 3]}}]}


def sweep_boxes():
    """Every box with corners from two pixels outside the frame to one past its far edge; of the boxes inverted along exactly one axis
    a third."""
    out = []
    for x0 in range(-2, SWEEP_W + 2):
        for x1 in range(-2, SWEEP_W + 2):
            for y0 in range(-2, SWEEP_H + 2):
                for y1 in range(-2, SWEEP_H + 2):
                    if (x0 > x1) != (y0 > y1) and (x0 + y0) % 3 != 0:
                        continue
                    out.append((x0, y0, x1, y1))
    return out


def sweep_rows():
    return make_rows([(SWEEP_LABELS[i % 3], 0.5, b) for i, b in enumerate(sweep_boxes())])


@functools.lru_cache(maxsize=None)
def sweep_expected():
    """The literal oracle on the sweep, computed once per process: (pass, zones, hits[3] = boxes that meet each zone's polygon)."""
    alpha, cfg = sweep_alpha(), sweep_config()
    want_pass, want_zones = literal_verdict(literal_filters(cfg, alpha), sweep_rows())
    polys = oz.zone_polygons(alpha)
    hits = tuple(sum(1 for b in sweep_boxes() if oz.box_intersects_polygon(*b, poly)) for poly in polys)
    for a in (want_pass, want_zones):
        a.setflags(write=False)
    return want_pass, want_zones, hits


# ---- 2. the tables at the shapes where their kernels change --------------------------------------------------------------------
TABLE_SHAPES = ((1, 1), (2, 1), (1, 2), (255, 3), (256, 3), (257, 3), (3, 255), (3, 256), (3, 257), (513, 258))
LARGE_SHAPE = (3840, 2160)


def pixels_of_interest(W, H):
    """The four corners and the pixels on either side of x = 255 | 256 and y = 255 | 256 (thread 255 | 0 of neighbouring workgroups of
    `wz_k_sat_cols` -- one thread per table column -- and `wz_k_sat_rows`), where they exist; no pixel twice."""
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    px += [(x, H // 2) for x in (254, 255, 256) if x < W]
    px += [(W // 2, y) for y in (254, 255, 256) if y < H]
    return list(dict.fromkeys(px))


def pixel_probes(W, H, x, y, label):
    """Boxes around one set pixel and whether they hold it: [(row, hit), ...]."""
    out = [((x, y, x, y), True)]
    out += [((x + dx, y + dy, x + dx, y + dy), False) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))]
    out += [((0, y, W - 1, y), True), ((x, 0, x, H - 1), True), ((0, 0, W - 1, H - 1), True)]
    if y > 0:
        out.append(((0, 0, W - 1, y - 1), False))          # the frame without that row: what lies above it ...
    if y < H - 1:
        out.append(((0, y + 1, W - 1, H - 1), False))      # ... and below
    if x > 0:
        out.append(((0, 0, x - 1, H - 1), False))
    if x < W - 1:
        out.append(((x + 1, 0, W - 1, H - 1), False))
    return [((label, 0.5, b), hit) for b, hit in out]


def single_pixel_case(W, H):
    """(Camera, rows, hit[n]): one zone per pixel of interest, a single set pixel each; label k + 1 is allowed zone k + 1 alone."""
    px = pixels_of_interest(W, H)
    fill = np.zeros((len(px), H, W), np.uint8)
    allow = np.zeros((NUM_LABELS, len(px)), np.uint8)
    dets, hits = [], []
    for k, (x, y) in enumerate(px):
        fill[k, y, x] = 1
        allow[k + 1, k] = 1
        for d, hit in pixel_probes(W, H, x, y, k + 1):
            dets.append(d)
            hits.append(hit)
    return Camera.plain(W, H, fill, allow), make_rows(dets), np.array(hits, bool)


def corners_case(W, H):
    """(Camera, rows): ONE zone with the four corner pixels set, the probes of every corner, and the frame without its border."""
    fill = np.zeros((1, H, W), np.uint8)
    dets = []
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        fill[0, y, x] = 1
        dets += [d for d, _ in pixel_probes(W, H, x, y, 1)]
    dets += [(1, 0.5, (1, 1, W - 2, H - 2)), (1, 0.5, (1, 0, W - 2, H - 1)), (1, 0.5, (0, 1, W - 1, H - 2)),
             (1, 0.5, (W - 1, H - 1, W + 5, H + 5)), (1, 0.5, (W, H, W + 5, H + 5)), (1, 0.5, (-5, -5, 0, 0))]
    return Camera.plain(W, H, fill), make_rows(dets)


def seeded_plane_case(W, H, value=1, seed=0):
    """(Camera, rows): one zone of density 1 / 64 (fill byte `value`); 1 x 1 boxes on every pixel of a small frame, else 2000 seeded
    boxes, a quarter of them one pixel tall or wide."""
    rng = np.random.default_rng([seed, W, H])
    fill = ((rng.integers(0, 64, (1, H, W)) == 0) * value).astype(np.uint8)
    if W * H <= 771:
        dets = [(1, 0.5, (x, y, x, y)) for y in range(H) for x in range(W)]
    else:
        dets = []
        for i in range(2000):
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            x1, y1 = int(rng.integers(x0, min(W, x0 + 24))), int(rng.integers(y0, min(H, y0 + 24)))
            if i % 8 == 0:
                x1 = x0
            elif i % 8 == 4:
                y1 = y0
            dets.append((1, 0.5, (x0, y0, x1, y1)))
    return Camera.plain(W, H, fill), make_rows(dets)


def plane_stride_case():
    """(Camera, rows, zones[n, 10]): 40 planes of 64 x 5, plane z with the one pixel (z, z % 5)."""
    W, H = 64, 5
    fill = np.zeros((CAM_ZONES, H, W), np.uint8)
    dets, want = [], []
    for z in range(CAM_ZONES):
        fill[z, z % H, z] = 1
        dets.append((1, 0.5, (z, z % H, z, z % H)))
        want.append([z + 1])
    dets += [(1, 0.5, (0, 0, W - 1, H - 1)), (1, 0.5, (30, 0, 39, H - 1)), (1, 0.5, (39, 0, W - 1, H - 1)), (1, 0.5, (40, 0, W - 1, H - 1))]
    want += [list(range(1, 11)), list(range(31, 41)), [40], []]
    zones = np.zeros((len(dets), ROW_ZONES), np.int32)
    for i, w in enumerate(want):
        zones[i, :len(w)] = w
    return Camera.plain(W, H, fill), make_rows(dets), zones


# ---- 3. zone cap and allow-lists -----------------------------------------------------------------------------------------------
CAP_W, CAP_H = 166, 30


def cap_alpha(blocks=CAM_ZONES):
    a = np.full((CAP_H, CAP_W), 100, np.uint8)
    for k in range(blocks):
        a[3:6, 4 * k + 1:4 * k + 3] = 255
    return a


def cap_config():
    return {"width": CAP_W, "height": CAP_H,
            "detect": [{"person": {"area": 0, "confidence": 0, "zones": []}},
                       {"car": {"area": 0, "confidence": 0, "zones": [3, 7] + list(range(12, 26))}},
                       {"truck": {"area": 0, "confidence": 0, "zones": [40]}}]}


def cap_rows():
    """(rows, zones expected by construction): block k (zone k) covers columns 4k - 3 and 4k - 2, rows 3 .. 5."""
    frame = (0, 0, CAP_W - 1, CAP_H - 1)
    cases = [((1, 0.5, frame), list(range(1, 11))),
             ((1, 0.5, (57, 0, CAP_W - 1, CAP_H - 1)), list(range(15, 25))),            # blocks 15 .. 40
             ((3, 0.5, frame), [3, 7] + list(range(12, 20))),
             ((8, 0.5, frame), [40]),
             ((8, 0.5, (0, 0, 156, CAP_H - 1)), []),                                    # everything but block 40
             ((1, 0.5, (17, 0, 54, CAP_H - 1)), list(range(5, 15))),                    # exactly 10 blocks
             ((1, 0.5, (17, 0, 57, CAP_H - 1)), list(range(5, 15))),                    # exactly 11: the 11th is not reported
             ((1, 0.5, (18, 5, 53, 5)), list(range(5, 15))),                            # the same 10 by their last row and edge columns
             ((1, 0.5, (3, 0, 4, CAP_H - 1)), []),                                      # between two blocks
             ((1, 0.5, (0, 6, CAP_W - 1, CAP_H - 1)), []),                              # under all of them
             ((3, 0.5, (0, 0, 43, CAP_H - 1)), [3, 7]),                                 # blocks 1 .. 11 through the allow-list
             ((3, 0.5, (0, 0, 8, CAP_H - 1)), []),                                      # blocks 1, 2: none allowed
             ((3, 0.5, (97, 0, CAP_W - 1, CAP_H - 1)), [25]),                           # blocks 25 .. 40: the list's last entry
             ((1, 0.5, (CAP_W - 1, 0, 0, CAP_H - 1)), list(range(1, 11)))]              # the frame, inverted
    zones = np.zeros((len(cases), ROW_ZONES), np.int32)
    for i, (_, w) in enumerate(cases):
        zones[i, :len(w)] = w
    return make_rows([c for c, _ in cases]), zones


# ---- 4. thresholds and labels --------------------------------------------------------------------------------------------------
EDGE_W = EDGE_H = 100


def edge_alpha():
    a = np.full((EDGE_H, EDGE_W), 100, np.uint8)
    a[0:40, 0:40] = 255
    a[60:90, 60:90] = 255
    return a


def threshold_config():
    """area 1 % of 100 x 100 = 100.0, 100 % = 10000.0"""
    return {"width": EDGE_W, "height": EDGE_H,
            "detect": [{"person": {"area": 1, "confidence": 50, "zones": []}},
                       {"car": {"area": 0, "confidence": 30, "zones": []}},
                       {"truck": {"area": 0, "confidence": 0, "zones": []}},
                       {"bench": {"area": 100, "confidence": 0, "zones": []}},
                       {"toothbrush": {"area": 0, "confidence": 0, "zones": [2]}}]}


def threshold_rows():
    """(rows, groups): groups = name -> row indices; both verdicts must occur in every group (in those named "mask: ..." on a
    camera with edge_alpha() as its mask)."""
    one = np.float32(1.0)
    lo = np.float32(0.0)
    h, t = np.float32(0.5), np.float32(0.3)
    box = (0, 0, 19, 19)                                   # area 400, inside the first zone of edge_alpha()
    groups, dets = {}, []

    def group(name, items):
        groups[name] = list(range(len(dets), len(dets) + len(items)))
        dets.extend(items)

    group("confidence 50", [(1, f32(v), box) for v in (np.nextafter(h, lo), h, np.nextafter(h, one))])
    group("confidence 30", [(3, f32(v), box) for v in (np.nextafter(t, lo), t, np.nextafter(t, one))])
    group("confidence 0", [(8, v, box) for v in (0.0, -0.0, float("nan"), float("inf"), float("-inf"), f32(-1e-45))])
    group("confidence 50, not finite", [(1, v, box) for v in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0)])
    group("area 100", [(1, 0.9, b) for b in ((0, 0, 9, 9), (0, 0, 8, 10), (0, 0, 100, 0), (0, 0, 10, 8), (0, 0, 99, 0))])
    group("area 0", [(3, 0.9, (5, 5, 4, 9)), (8, 0.9, (5, 5, 4, 4)), (1, 0.9, (5, 5, 4, 9)), (1, 0.9, (5, 5, 4, 4))])
    group("both extents negative", [(1, 0.9, (20, 20, 9, 9)), (1, 0.9, (20, 20, 10, 9)), (1, 0.9, (20, 20, 9, 10))])
    group("one extent negative", [(1, 0.9, (20, 0, 9, 11)), (1, 0.9, (20, 0, 9, 8)), (1, 0.9, (0, 20, 11, 9)), (1, 0.9, (0, 20, 8, 9))])
    group("area 10000", [(15, 0.9, b) for b in ((0, 0, 99, 99), (0, 0, 99, 98), (0, 0, 100, 98), (99, 99, 0, 0), (-1, 0, 99, 98),
                                                      (-1, 0, 99, 99), (100, 100, -1, -1))])
    group("labels", [(l, 0.9, box) for l in (0, -1, 1, 90, 91, 1000, 2, 8, 89, I32_MIN, I32_MAX)])
    group("mask: zone allowed", [(90, 0.9, (70, 70, 80, 80)), (90, 0.9, box), (8, 0.9, (45, 45, 55, 55)), (8, 0.9, (39, 39, 60, 60))])
    return make_rows(dets), groups


# ---- 5. wild coordinates -------------------------------------------------------------------------------------------------------
def wild_config():
    return {"width": EDGE_W, "height": EDGE_H,
            "detect": [{"person": {"area": 0, "confidence": 0, "zones": []}},
                       {"car": {"area": 1, "confidence": 0, "zones": []}},
                       {"bench": {"area": 100, "confidence": 0, "zones": []}}]}


def wild_rows():
    """(rows, groups): every box under the three labels of wild_config().  Without a mask nothing fails an area threshold of 0."""
    boxes = [(I32_MIN, 0, I32_MAX, 0),
             (0, 0, I32_MAX, I32_MAX),
             (-1, -1, I32_MAX - 1, 5),
             (I32_MAX, I32_MAX, I32_MIN, I32_MIN),
             (I32_MIN, I32_MIN, I32_MAX, I32_MAX),
             (-50, 10, -1, 20), (100, 10, 150, 20), (10, -30, 20, -1), (10, 100, 20, 2000),          # left, right, above, below
             (I32_MIN, 0, I32_MIN + 5, 5), (I32_MAX - 5, 0, I32_MAX, 5), (0, I32_MIN, 5, I32_MIN + 5), (0, I32_MAX - 5, 5, I32_MAX),
             (-10 ** 9, -10 ** 9, 10 ** 9, 10 ** 9),                                                 # the frame from far outside
             (I32_MIN, 45, I32_MAX, 55), (45, I32_MIN, 55, I32_MAX),                                  # bands between the zones
             (I32_MIN, I32_MAX, I32_MAX, I32_MIN), (I32_MAX, 39, I32_MIN, 39), (39, I32_MAX, 40, I32_MIN),
             (I32_MIN, I32_MIN, -1, I32_MAX), (I32_MIN, 0, I32_MAX, 1), (-2, 0, I32_MAX, 0)]
    groups, dets = {}, []
    for name, label in (("mask: area 0", 1), ("area 100", 3), ("area 10000", 15)):
        groups[name] = list(range(len(dets), len(dets) + len(boxes)))
        dets += [(label, 0.9, b) for b in boxes]
    return make_rows(dets), groups
