"""Engines come and go: what an engine allocates on the device leaves with it, whichever entry points it served."""
import json
import os
import subprocess
import sys

import pytest

import conftest

pytestmark = pytest.mark.gpu

MIB = 1 << 20

# The same child (CHILD below) on the commit before the engine's blocks got owners, on an MI355X: the free device
# memory after the first close minus that after the fourth, and what one open engine (max batch 2, 640 x 480, every lazy share allocated)
# takes from the device.  profiles/lane_owners_lifecycle.txt has both runs.
PARENT_LOST_1_TO_4 = 0
PARENT_OPEN_BYTES = 404750336

# argv: repository root, engine file.  Prints one JSON line: free bytes after every close, free bytes with every engine open (just before
# its close) and just before its wz_create.
CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from watsor_amd.runtime import HipEngine, ROW_DTYPE
from watsor_amd.synth import synthetic_frame

hip = None
def free_bytes():
    global hip
    if hip is None:      # the HIP runtime the library itself loaded (one runtime per process)
        path = [l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l][0]
        hip = C.CDLL(path)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)

W, H = 640, 480
frames = [synthetic_frame(W, H, 9700 + i) for i in range(2)]
after_close, opened, before = [], [], []
for r in range(4):
    if r:
        before.append(free_bytes())
    e = HipEngine(sys.argv[2], 0, 2, W, H)
    rows = [np.zeros(100, ROW_DTYPE) for _ in frames]
    for slot in range(e.num_slots):                      # one plain batch on every lane
        e.submit_host(slot, frames)
        e.collect(slot, rows)
    halves = [(0, 0, 320, 480), (320, 0, 320, 480)]
    e.detect_tiled(frames[:1], [halves], rows[:1])      # tiled, gated and motion with a hold: lane 0's lazy shares, the cameras' state
    e.set_camera_tiles(1, W, H, halves, 8)
    e.detect_gated(frames[:1], [1], rows[:1])
    e.set_camera_motion(2, W, H, 8, max_regions=1)
    e.set_camera_motion_hold(2, hold=2, object_hold=1)
    e.detect_motion(frames[:1], [2], rows[:1])
    e.detect_motion(frames[1:], [2], rows[:1])
    zones = np.zeros((2, H, W), np.uint8)                # a camera filter with a zone mask: the summed-area tables
    zones[0, :240] = 1
    zones[1, 240:, 320:] = 1
    e.set_camera_filter(3, W, H, np.full(91, 0.3), np.full(91, 0.0), zones, np.ones((91, 2), np.uint8))
    e.detect_batch(frames, rows, cams=[3, 3])
    e.sync()
    opened.append(free_bytes())
    e.close()
    after_close.append(free_bytes())
print(json.dumps(dict(after_close=after_close, opened=opened, before=before)))
"""


def test_engines_come_and_go(model_dir_robust):
    """One process creates an engine (max batch 2, 640 x 480), runs a plain batch on every lane, a tiled, a gated and a motion call with a
    hold on lane 0, sets a camera filter with a zone mask, and closes it -- four times.  The device's free memory after the fourth close
    is what it was after the first (the first close leaves the runtime's own pools and the loaded code behind, the later ones nothing more):
    the bar is the figure the same child gave on the commit before the blocks had owners, plus 1 MiB.  Every block this can catch is far
    larger than that -- activation slots, the 64 MiB workspace, 0.9 MB of staging a frame, the summed-area tables.  The small blocks are
    not covered by this test: that no free is written by hand any more (wz_engine.hip holds no hipFree / hipHostFree of a lane's or the
    engine's block, they live in the owners of wz_engine.h) is what covers them.
    An open engine also takes LESS than it did then: the engine-wide second staging area (max_batch * frame_stride bytes) and the two
    device row blocks per lane that no batch ever wrote are gone."""
    p = subprocess.run([sys.executable, "-c", CHILD, conftest.ROOT, os.path.join(model_dir_robust, "mi355x.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    lost = out["after_close"][0] - out["after_close"][3]
    open_bytes = [b - o for b, o in zip(out["before"], out["opened"][1:])]       # engines 2 .. 4: the runtime's one-off costs are paid
    print("free after close 1 - after close 4: %d bytes (parent %d); an open engine takes %s bytes (parent %d)"
          % (lost, PARENT_LOST_1_TO_4, open_bytes, PARENT_OPEN_BYTES))
    assert lost <= PARENT_LOST_1_TO_4 + MIB
    assert max(open_bytes) < PARENT_OPEN_BYTES
