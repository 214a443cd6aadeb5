"""Four lanes on hardware queues of their own where the host pinned GPU_MAX_HW_QUEUES=4 (include/watsor_hip.h: wz_hw_queues): the library
takes 8, and four batches in flight on four lanes give bit for bit the rows each of them gives alone (the
run-to-run criterion of the soak).  Then the product ABI's synchronous copies, which ride lane 0's stream: an upload, a download and
a camera filter set while every lane is busy.  One fresh child process (the variable counts before the process's first HIP call)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from oracle import filters as of
from watsor_amd import runtime
from watsor_amd.coco import COCO_CLASSES
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import HipEngine, ROW_DTYPE
from watsor_amd.share import BoundingBox, Detection
from watsor_amd.synth import synthetic_frame, synthetic_zone_mask

W, H = 640, 480
before = runtime.hw_queues()
eng = HipEngine(sys.argv[2], 0, 2, W, H)
after, lanes = runtime.hw_queues(), eng.num_slots
assert (before, after, lanes) == (8, 8, 4), (before, after, lanes)

frames = [synthetic_frame(W, H, 500 + i) for i in range(6)]
d = [eng.upload(f) for f in frames]
batches = [[0], [1, 2], [3, 4], [5]]                      # sizes 1, 2, 2, 1: four different batches


def submit(lane, ptrs, cams=None):
    eng.submit_device(lane, ptrs, [W] * len(ptrs), [H] * len(ptrs), cams=cams)


def rows_of(lane, n):
    eng.wait(lane)
    return eng.slot_rows(lane, n).copy()


together = []
for rnd in range(3):
    for lane, b in enumerate(batches):                    # back to back: all four in flight
        submit(lane, [d[i] for i in b])
    together.append([rows_of(lane, len(b)) for lane, b in enumerate(batches)])
alone = []
for b in batches:
    submit(0, [d[i] for i in b])
    alone.append(rows_of(0, len(b)))
for b, rows in zip(batches, alone):
    assert (rows["label"] >= 1).any(), "batch %s detected nothing: the comparison would be empty" % b
for rnd, got in enumerate(together):
    for lane, (b, rows) in enumerate(zip(batches, got)):
        assert rows.tobytes() == alone[lane].tobytes(), "round %d, lane %d (frames %s): rows differ from the batch's lone run" % (rnd, lane, b)
print("lanes: 3 rounds x 4 batches in flight == alone")

# an upload, a download and a camera filter while all four lanes are busy
cfg = {"width": W, "height": H, "detect": [{name: {"area": 1, "confidence": 10, "zones": []}}      # (the seeded random-init network mostly
                                             for name in ("person", "car", COCO_CLASSES[14])]}       #  reports label 14: let it through)
alpha = synthetic_zone_mask(W, H, 77, 4)
extra = synthetic_frame(W, H, 900)
for lane, b in enumerate(batches):
    submit(lane, [d[i] for i in b])
p = eng.upload(extra)
back = eng.download(p, extra.nbytes)
flt = HipCameraFilter(eng, 5, cfg, alpha=alpha)
busy = [rows_of(lane, len(b)) for lane, b in enumerate(batches)]
assert back.tobytes() == extra.tobytes(), "bytes downloaded differ from the bytes uploaded while the lanes were busy"
for lane, rows in enumerate(busy):
    assert rows.tobytes() == alone[lane].tobytes(), "lane %d: rows differ after an upload and a filter set in mid-flight" % lane

rows = [np.zeros(100, ROW_DTYPE) for _ in range(2)]
passes = [np.full(100, 9, np.uint8) for _ in range(2)]
submit(1, [p, d[0]], cams=[5, -1])                        # the next batch: the new frame under the new filter, an old one without
eng.collect(1, rows, passes)
filters = [of.ConfidenceFilter(cfg), of.AreaFilter(cfg), of.MaskFilter(cfg, alpha=alpha)]
want_pass, want_zones = np.zeros(100, np.uint8), np.zeros((100, 10), np.int32)
for i in range(100):
    r = rows[0][i]
    det = Detection(label=int(r["label"]), confidence=float(r["confidence"]),
                    bounding_box=BoundingBox(int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])))
    want_pass[i] = 1 if (det.label > 0 and all(f(det) for f in filters)) else 0
    want_zones[i] = list(det.zones)
np.testing.assert_array_equal(passes[0], want_pass)
np.testing.assert_array_equal(rows[0]["zones"], want_zones)
assert (want_zones > 0).any(), "no row of the new frame lies in a zone: the zones[] check would be empty"
assert not rows[1]["zones"].any()
np.testing.assert_array_equal(passes[1], (rows[1]["label"] > 0).astype(np.uint8))
submit(0, [p, d[0]])                                      # the same batch without the filter, the lanes idle: the rows but for zones[]
ref = rows_of(0, 2)
got = rows[0].copy()
got["zones"] = 0
assert got.tobytes() == ref[0].tobytes() and rows[1].tobytes() == ref[1].tobytes(), "the uploaded frame's rows differ from its lone run"
flt.close()
eng.close()
print("copies on lane 0: upload, download and filter in mid-flight are right")
print("OK")
"""


def test_four_lanes_on_eight_queues_where_the_host_pinned_four(model_dir_robust):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(model_dir_robust, "mi355x.bin")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
