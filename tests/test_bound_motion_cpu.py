"""Motion regions through the worker's frame table, the parts that need no GPU: `plan_bound` (watsor_amd/detection/hip_gpu.py) cuts motion
entries like gated ones -- one kind and one pair of thresholds per call, the cameras' configured whole_frame + max_regions within max_batch,
one frame of a camera per call -- and `BatchedWorkerMixin` under `hip_tiled_table=True` binds the tiled table for a detector that says
`motion` and submits the pieces on successive lanes, one latch step per payload."""
import shm_standins as shm
from test_worker_logic import TableDetector, Worker, drive, first_row, setup
from watsor_amd import _lib
from watsor_amd.detection.hip_gpu import HipObjectDetector, plan_bound


def motion(n, cam, iou=0.6, ios=1.0):
    return ("motion", iou, ios, n, cam)


def gated(n, cam, iou=0.6, ios=1.0):
    return ("gated", iou, ios, n, cam)


def tiled(n, cam=-1, iou=0.6, ios=1.0):
    return ("tiled", iou, ios, n, cam)


PLAIN = ("plain", None, None, 1, -1)


# ---- plan_bound: known answers ------------------------------------------------------------------------------------------------------------
def test_two_frames_of_one_motion_camera_make_two_calls():
    d = [motion(3, 0), motion(3, 0), motion(3, 1)]
    assert plan_bound(d, [0, 1], 8) == [[0], [1]]
    assert plan_bound(d, [0, 2, 1], 8) == [[0, 2], [1]]           # another camera shares the call, the second frame of camera 0 opens the next
    assert plan_bound(d, [1, 0], 8) == [[1], [0]]


def test_the_configured_counts_are_summed_as_the_engine_sums_them():
    d = [motion(4, 0), motion(4, 1), motion(4, 2)]
    assert plan_bound(d, [0, 1, 2], 8) == [[0, 1], [2]]           # 4 + 4 fit exactly, the third camera's 4 do not
    assert [len(c) for c in plan_bound(d, [0, 1, 2], 8)] == [2, 1]
    assert plan_bound([motion(5, 0), motion(5, 1)], [0, 1], 8) == [[0], [1]]


def test_two_threshold_pairs_split_a_motion_batch():
    d = [motion(2, 0), motion(2, 1, iou=0.5), motion(2, 2), motion(2, 3, ios=0.7)]
    assert plan_bound(d, [0, 2, 1, 3], 8) == [[0, 2], [1], [3]]
    assert plan_bound(d, [0, 1, 2], 8) == [[0], [1], [2]]         # consecutive pieces: nothing is reordered to fill a call


def test_motion_beside_plain_tiled_and_gated_entries_keeps_one_kind_per_call_and_the_order():
    d = [PLAIN, motion(3, 5), tiled(3), gated(3, 4), motion(3, 6), PLAIN, motion(3, 5)]
    entries = [0, 5, 1, 4, 2, 3, 6, 1]
    calls = plan_bound(d, entries, 8)
    assert calls == [[0, 5], [1, 4], [2], [3], [6], [1]]          # (6 and 1 are both camera 5's: two calls)
    assert [i for c in calls for i in c] == entries
    for c in calls:
        assert len({d[i][0] for i in c}) == 1 and sum(d[i][3] for i in c) <= 8
    # the same thresholds and the same camera under another kind do not join a motion call
    assert plan_bound([motion(2, 4), gated(2, 4), motion(2, 7)], [0, 1, 2], 8) == [[0], [1], [2]]


def test_the_plugin_plans_motion_entries_from_its_bound_descriptions():
    det = HipObjectDetector.__new__(HipObjectDetector)           # (no engine: planning reads the recorded descriptions only)
    det.bound_descriptions = [motion(4, 0), motion(4, 0), motion(4, 1), motion(4, 2)]
    det.bound_max_batch = 8
    assert det.plan_bound([0, 2, 3, 1]) == [[0, 2], [3, 1]]
    assert det.plan_bound([0, 1, 2]) == [[0], [1, 2]]


def test_the_binding_and_the_header_agree_on_wz_bind_motion():
    import os
    import re
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "watsor_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bwz_bind_motion\s*\(([^)]*)\)", header)
    assert m and len(_lib.SIGNATURES["wz_bind_motion"][1]) == len(m.group(1).split(",")) == 5
    assert getattr(_lib.load(), "wz_bind_motion") and getattr(_lib.load(dev=True), "wz_bind_motion")


# ---- the worker -----------------------------------------------------------------------------------------------------------------------------
class MotionTableDetector(TableDetector):
    """A detector with a `motion` option and no tiles, whose tiled frame table binds every camera's frames as motion entries: cam0 and cam1
    with 3 configured tiles, cam2 with 5."""
    motion = True
    max_batch = 8
    num_lanes = 3

    def submit_host(self, lane, images, cameras=None):
        raise AssertionError("the asynchronous host path detects untiled")

    def bind_frame_table(self, frame_buffers, ids):
        raise AssertionError("the untiled frame table of a motion detector")

    def bind_tiled_frame_table(self, frame_buffers, ids):
        table = TableDetector.bind_frame_table(self, frame_buffers, ids)
        self.descriptions = []
        for name in sorted(frame_buffers):
            self.descriptions += [motion(5 if name == "cam2" else 3, ids[name])] * len(frame_buffers[name].frames)
        return table

    def plan_bound(self, entries):
        calls = plan_bound(self.descriptions, entries, self.max_batch)
        self.log.append(("plan", [list(c) for c in calls]))
        return calls


def test_worker_binds_the_tiled_table_for_a_motion_detector_and_submits_the_pieces_on_successive_lanes():
    _, cams = setup()
    det, w = MotionTableDetector(), Worker()
    batches = [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(4)]
    fps, it = drive(w, det, cams, batches, hip_tiled_table=True, hip_metric_interval=0)
    st = w._hip_worker_state
    assert st["asynchronous"] and st["plan"] is not None and st["table"] is not None
    assert ("table", 12) in det.log and not [e for e in det.log if e[0] in ("submit", "sync")]      # detect_batch was never called
    # cam c, frame i -> 4 c + i; a batch [cam0: 3, cam1: 3, cam2: 5] is two calls: 3 + 3 + 5 > 8
    plans = [e[1] for e in det.log if e[0] == "plan"]
    assert plans == [[[i, 4 + i], [8 + i]] for i in range(4)]
    subs = [e for e in det.log if e[0] == "submit_bound"]
    assert [e[2] for e in subs] == [p for plan in plans for p in plan]
    assert [e[1] for e in subs] == [k % 3 for k in range(8)]                # successive lanes, round robin over the three
    assert det.max_in_flight <= 3 and not det.busy                        # (TableDetector asserts that no lane is reused before its collect)
    for c in range(3):
        for i in range(4):
            f = cams["cam%d" % c].frames[i]
            assert first_row(f) == (1 + 10 * c + i, c)                    # rows in the frame's own header
            assert f.latch.steps.value == 1                               # every payload's latch once
    assert fps.count.value == 12 and it.count.value == 8                  # one observation per piece


def test_two_frames_of_a_motion_camera_in_one_batch_go_to_two_lanes_in_order():
    _, cams = setup()
    det, w = MotionTableDetector(), Worker()
    drive(w, det, cams, [[shm.Payload("cam0", 0), shm.Payload("cam0", 1), shm.Payload("cam1", 2)]], hip_tiled_table=True)
    assert [e[1:] for e in det.log if e[0] == "submit_bound"] == [(0, [0]), (1, [1, 6])]
    assert [cams["cam0"].frames[i].latch.steps.value for i in range(2)] == [1, 1] and cams["cam1"].frames[2].latch.steps.value == 1


def test_a_motion_table_that_cannot_be_bound_takes_the_synchronous_path_and_never_submit_host():
    _, cams = setup()

    class Refusing(MotionTableDetector):
        def bind_tiled_frame_table(self, frame_buffers, ids):
            raise ValueError("camera 'cam1': the frames of a motion camera must share one size and format")

    det, w = Refusing(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(2)], hip_tiled_table=True, hip_metric_interval=0)
    assert not w._hip_worker_state["asynchronous"]
    assert [e for e in det.log if e[0] == "sync"] == [("sync", 3), ("sync", 3)]
    assert not [e for e in det.log if e[0] in ("submit", "submit_bound", "table")]
    assert all(first_row(cams["cam%d" % c].frames[i]) == (1 + 10 * c + i, c) for c in range(3) for i in range(2))
    assert all(cams["cam%d" % c].frames[i].latch.steps.value == 1 for c in range(3) for i in range(2))


def test_a_refused_motion_piece_is_retried_synchronously_with_the_pieces_behind_it():
    _, cams = setup()

    class RefusingSecond(MotionTableDetector):
        def submit_bound(self, lane, entries):
            if entries == [1, 5]:
                raise ValueError("frame 0: camera 0 has no motion settings (wz_set_camera_motion first)")
            super().submit_bound(lane, entries)

    det, w = RefusingSecond(), Worker()
    batch = [shm.Payload("cam0", 0), shm.Payload("cam0", 1), shm.Payload("cam1", 1), shm.Payload("cam2", 1)]
    fps, _ = drive(w, det, cams, [batch], hip_tiled_table=True)
    assert [e for e in det.log if e[0] == "plan"] == [("plan", [[0], [1, 5], [9]])]
    assert [e[2] for e in det.log if e[0] == "submit_bound"] == [[0]]
    order = [e[0] for e in det.log if e[0] in ("submit_bound", "collect_bound", "sync")]
    assert order == ["submit_bound", "collect_bound", "sync"]               # what was in flight is retired first: the camera's order is kept
    assert ("sync", 3) in det.log                                            # the refused piece and the one behind it, synchronously
    assert first_row(cams["cam0"].frames[0]) == (1, 0) and first_row(cams["cam0"].frames[1]) == (2, 0)
    assert first_row(cams["cam1"].frames[1]) == (12, 1) and first_row(cams["cam2"].frames[1]) == (22, 2)
    assert [cams[n].frames[i].latch.steps.value for n, i in (("cam0", 0), ("cam0", 1), ("cam1", 1), ("cam2", 1))] == [1, 1, 1, 1]
    assert fps.count.value == 4


def test_without_the_option_a_motion_detector_stays_synchronous():
    _, cams = setup()
    det, w = MotionTableDetector(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, 0) for c in range(3)]])
    assert ("sync", 3) in det.log and not [e for e in det.log if e[0] in ("table", "plan", "submit_bound")]
    det, w = MotionTableDetector(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, 1) for c in range(3)]], hip_tiled_table=True, hip_frame_table=False)
    assert ("sync", 3) in det.log and not [e for e in det.log if e[0] in ("table", "plan", "submit_bound")]
