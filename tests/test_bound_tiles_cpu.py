"""Tiled and gated detection through the worker's frame table, the parts that need no GPU: `plan_bound` (watsor_amd/detection/hip_gpu.py)
cuts a list of table indices into the calls `wz_submit_bound` accepts, and `BatchedWorkerMixin` under `hip_tiled_table=True` submits those
pieces on successive lanes, one latch step per payload."""
import numpy as np

import shm_standins as shm
from test_worker_logic import TableDetector, Worker, drive, first_row, setup
from watsor_amd import _lib
from watsor_amd.detection.hip_gpu import HipObjectDetector, plan_bound


def tiled(n, cam=-1, iou=0.6, ios=1.0):
    return ("tiled", iou, ios, n, cam)


def gated(n, cam, iou=0.6, ios=1.0):
    return ("gated", iou, ios, n, cam)


PLAIN = ("plain", None, None, 1, -1)


# ---- plan_bound: known answers ------------------------------------------------------------------------------------------------------------
def test_tiles_beyond_max_batch_make_two_calls():
    assert plan_bound([tiled(5), tiled(5)], [0, 1], 8) == [[0], [1]]
    assert plan_bound([tiled(4), tiled(4), tiled(1)], [0, 1, 2], 8) == [[0, 1], [2]]         # 4 + 4 fit exactly, the ninth tile does not
    assert plan_bound([PLAIN] * 10, list(range(10)), 8) == [list(range(8)), [8, 9]]         # untiled: max_batch frames


def test_two_frames_of_one_gated_camera_make_two_calls_in_order():
    d = [gated(2, 0), gated(2, 0), gated(2, 1)]
    assert plan_bound(d, [0, 1], 8) == [[0], [1]]
    assert plan_bound(d, [0, 2, 1], 8) == [[0, 2], [1]]           # another camera shares the call, the second frame of camera 0 opens the next
    assert plan_bound(d, [1, 0], 8) == [[1], [0]]
    # the CONFIGURED tile counts are summed, as the engine sums them
    assert plan_bound([gated(5, 0), gated(5, 1)], [0, 1], 8) == [[0], [1]]


def test_two_threshold_pairs_split_a_batch():
    d = [tiled(2), tiled(2, iou=0.5), tiled(2), tiled(2, ios=0.7)]
    assert plan_bound(d, [0, 2, 1, 3], 8) == [[0, 2], [1], [3]]
    assert plan_bound(d, [0, 1, 2], 8) == [[0], [1], [2]]         # consecutive pieces: nothing is reordered to fill a call


def test_untiled_and_tiled_split_a_batch():
    d = [PLAIN, tiled(3), PLAIN, gated(3, 4), tiled(3, cam=4)]
    assert plan_bound(d, [0, 2, 1, 4, 3], 8) == [[0, 2], [1, 4], [3]]
    assert plan_bound(d, [0, 1, 2], 8) == [[0], [1], [2]]
    assert plan_bound(d, [9, 0], 8) == [[9, 0]]                   # an index the table does not describe counts as untiled (the engine refuses it)
    assert plan_bound(d, [], 8) == []


def test_order_inside_a_camera_is_kept():
    d = [gated(3, 0)] * 3 + [gated(3, 1)] * 3 + [tiled(5, 2)] * 2
    entries = [0, 3, 6, 1, 4, 7, 2, 5]
    calls = plan_bound(d, entries, 8)
    assert [i for c in calls for i in c] == entries               # the calls are the list itself, cut
    assert calls == [[0, 3], [6], [1, 4], [7], [2, 5]]
    for c in calls:
        kinds = {d[i][0] for i in c}
        assert len(kinds) == 1 and sum(d[i][3] for i in c) <= 8
        assert kinds != {"gated"} or len({d[i][4] for i in c}) == len(c)


def test_the_plugin_plans_from_its_bound_descriptions():
    det = HipObjectDetector.__new__(HipObjectDetector)           # (no engine: planning reads the recorded descriptions only)
    det.bound_descriptions = [tiled(5), tiled(5), PLAIN]
    det.bound_max_batch = 8
    assert det.plan_bound([0, 1, 2, 2]) == [[0], [1], [2, 2]]


def test_the_binding_and_the_header_agree_on_wz_bind_tiles():
    import os
    import re
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "watsor_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, table in [("wz_bind_tiles", _lib.SIGNATURES), ("wz_debug_bound_source", _lib.DEV_SIGNATURES)]:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(table[name][1]) == len(m.group(1).split(",")), name
    assert getattr(_lib.load(), "wz_bind_tiles") and getattr(_lib.load(dev=True), "wz_debug_bound_source")
    assert not hasattr(_lib.load(), "wz_debug_bound_source")


# ---- the worker -----------------------------------------------------------------------------------------------------------------------------
class TiledTableDetector(TableDetector):
    """A detector with a `tiles` option and a tiled frame table: cam0 gated (2 tiles), cam1 tiled (5 tiles), cam2 tiled (5 tiles)."""
    tiled = True
    max_batch = 8
    num_lanes = 3

    def submit_host(self, lane, images, cameras=None):
        raise AssertionError("the asynchronous host path detects untiled")

    def bind_frame_table(self, frame_buffers, ids):
        raise AssertionError("the untiled frame table of a tiled detector")

    def bind_tiled_frame_table(self, frame_buffers, ids):
        table = TableDetector.bind_frame_table(self, frame_buffers, ids)
        self.descriptions = []
        for name in sorted(frame_buffers):
            n = len(frame_buffers[name].frames)
            self.descriptions += [gated(2, ids[name]) if name == "cam0" else tiled(5, ids[name])] * n
        return table

    def plan_bound(self, entries):
        calls = plan_bound(self.descriptions, entries, self.max_batch)
        self.log.append(("plan", [list(c) for c in calls]))
        return calls


def test_worker_submits_the_planned_pieces_on_successive_lanes():
    _, cams = setup()
    det, w = TiledTableDetector(), Worker()
    batches = [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(4)]
    fps, it = drive(w, det, cams, batches, hip_tiled_table=True, hip_metric_interval=0)
    assert ("table", 12) in det.log and not [e for e in det.log if e[0] in ("submit", "sync")]
    # cam c, frame i -> 4 c + i; a batch [cam0 gated, cam1 tiled 5, cam2 tiled 5] is three calls: the kind changes, then 5 + 5 > 8
    plans = [e[1] for e in det.log if e[0] == "plan"]
    assert plans == [[[i], [4 + i], [8 + i]] for i in range(4)]
    subs = [e for e in det.log if e[0] == "submit_bound"]
    assert [e[2] for e in subs] == [p for plan in plans for p in plan]
    assert [e[1] for e in subs] == [k % 3 for k in range(12)]               # successive lanes, round robin over the three
    assert det.max_in_flight <= 3 and not det.busy                        # (TableDetector asserts that no lane is reused before its collect)
    for c in range(3):
        for i in range(4):
            f = cams["cam%d" % c].frames[i]
            assert first_row(f) == (1 + 10 * c + i, c)                    # rows in the frame's own header
            assert f.latch.steps.value == 1                               # every payload's latch once
    assert fps.count.value == 12 and it.count.value == 12                 # one observation per piece


def test_worker_with_fewer_lanes_than_pieces_retires_the_oldest_first():
    _, cams = setup()
    det, w = TiledTableDetector(), Worker()
    batch = [shm.Payload("cam%d" % c, 0) for c in range(3)] + [shm.Payload("cam1", 1), shm.Payload("nobody", 0)]
    drive(w, det, cams, [batch], hip_tiled_table=True, hip_lanes=2)
    order = [e[:2] for e in det.log if e[0] in ("submit_bound", "collect_bound")]
    assert order == [("submit_bound", 0), ("submit_bound", 1), ("collect_bound", 0), ("submit_bound", 0), ("collect_bound", 1), ("submit_bound", 1),
                     ("collect_bound", 0), ("collect_bound", 1)]
    assert det.max_in_flight == 2
    assert [cams["cam%d" % c].frames[0].latch.steps.value for c in range(3)] == [1, 1, 1] and cams["cam1"].frames[1].latch.steps.value == 1
    assert first_row(cams["cam1"].frames[1]) == (12, 1)


def test_a_refused_piece_is_retried_synchronously_and_every_latch_steps_once():
    _, cams = setup()

    class RefusingSecond(TiledTableDetector):
        def submit_bound(self, lane, entries):
            if entries == [4]:
                raise ValueError("9 tiles in one call exceed max_batch 8")
            super().submit_bound(lane, entries)

    det, w = RefusingSecond(), Worker()
    fps, _ = drive(w, det, cams, [[shm.Payload("cam%d" % c, 0) for c in range(3)]], hip_tiled_table=True)
    assert [e[2] for e in det.log if e[0] == "submit_bound"] == [[0]]
    assert ("sync", 2) in det.log                                            # the refused piece and the one behind it, synchronously
    assert all(first_row(cams["cam%d" % c].frames[0]) == (1 + 10 * c, c) for c in range(3))
    assert [cams["cam%d" % c].frames[0].latch.steps.value for c in range(3)] == [1, 1, 1] and fps.count.value == 3


def test_a_refused_tiled_table_takes_the_synchronous_path_and_never_submit_host():
    _, cams = setup()

    class Refusing(TiledTableDetector):
        def bind_tiled_frame_table(self, frame_buffers, ids):
            raise ValueError("camera 'cam1': tile 3 (600, 0, 100 x 48): the rectangle leaves the frame")

    det, w = Refusing(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(2)], hip_tiled_table=True, hip_metric_interval=0)
    assert [e for e in det.log if e[0] == "sync"] == [("sync", 3), ("sync", 3)]
    assert not [e for e in det.log if e[0] in ("submit", "submit_bound", "table")]
    assert all(first_row(cams["cam%d" % c].frames[i]) == (1 + 10 * c + i, c) for c in range(3) for i in range(2))
    assert all(cams["cam%d" % c].frames[i].latch.steps.value == 1 for c in range(3) for i in range(2))


def test_without_the_option_a_tiled_detector_stays_synchronous():
    _, cams = setup()
    det, w = TiledTableDetector(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, 0) for c in range(3)]])
    assert ("sync", 3) in det.log and not [e for e in det.log if e[0] in ("table", "plan", "submit_bound")]
    # ... and an untiled detector ignores the option: its table is the plain one
    det, w = TableDetector(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, 1) for c in range(3)]], hip_tiled_table=True)
    assert [e[2] for e in det.log if e[0] == "submit_bound"] == [[1, 5, 9]]
    assert np.frombuffer(cams["cam0"].frames[1].image.get_obj(), np.uint8)[0] == 1
