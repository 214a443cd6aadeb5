"""The network enqueue launches what tests/golden/network_launches.json recorded (tests/launch_golden.py: the cases and what a
recording holds): the same kernels with the same grids, blocks and LDS in the same order, the same graph, the same post-processing
flags, the same stage names and -- the launches' ARGUMENTS -- the same rows bit for bit, for every engine program at batches 1, 2, 3
and 8, captured and kernel by kernel, and under each knob that takes another way through the enqueue.  Equality throughout: the
recording comes from the commit before the enqueue was last restructured and is only ever made again from such a parent.

And the stage profile (wz_profile_stages), whose own check is that the batch recorded one mark per stage: every program, batch 1 and 8."""
import json
import os

import numpy as np
import pytest

import launch_golden as lg
from watsor_amd.runtime import HipEngine
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_models")
    out = lg.build_models(d)
    with open(os.path.join(str(d), "models.json"), "w") as f:
        json.dump(out, f)
    return out


@pytest.fixture(scope="module")
def golden():
    return lg.golden()


@pytest.mark.parametrize("program,env", lg.CASES, ids=[lg.key(c) for c in lg.CASES])
def test_launches_match_the_recording(models, golden, tmp_path, program, env):
    if not os.path.isfile(lg.STAMPS):
        pytest.skip("no stamps build here (make -C watsor_amd/csrc stamps)")
    models_json = os.path.join(os.path.dirname(os.path.dirname(models[program])), "models.json")
    out_json = str(tmp_path / "out.json")
    p = lg.run_child(env, [program], models_json, out_json, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out_json) as f:
        got = json.load(f)[lg.key((program, env))]
    want = golden[lg.key((program, env))]
    assert got["stages"] == want["stages"]
    assert sorted(got["batches"]) == sorted(want["batches"]) == sorted(str(n) for n in lg.ENVIRONMENTS[env][2])
    for n, w in want["batches"].items():
        g = got["batches"][n]
        assert g["launches"] == w["launches"], "batch %s: launch %d differs" % (
            n, next((i for i, (a, b) in enumerate(zip(g["launches"], w["launches"])) if a != b), min(len(g["launches"]), len(w["launches"]))))
        assert g["graph_nodes"] == w["graph_nodes"], "batch %s" % n
        assert (g["decode_fused"], g["cands_listed"]) == (w["decode_fused"], w["cands_listed"]), "batch %s" % n
        # the same launches with other rows: other ARGUMENTS (a K split, a workspace offset, dup_k) -- a bug, never a reason to record again
        assert g["rows_sha256"] == w["rows_sha256"], "batch %s: the launches are the recorded ones, the rows are not" % n


def test_the_recording_holds_a_refused_parking(golden):
    """The twelve-head engine (launch_golden.PROGRAMS) is the case whose last heads find the grouped reduce full: its boxes are not
    all finished there, so the decode stays a launch of its own -- one graph node more than launches noted (wz_k_decode notes none)."""
    for env in ("graph", "kernel_by_kernel"):
        for n, b in golden["heads_twice/" + env]["batches"].items():
            assert not b["decode_fused"] and not b["cands_listed"], (env, n)
    assert all(b["decode_fused"] and b["cands_listed"] for b in golden["default/graph"]["batches"].values())
    assert len(golden["heads_twice/graph"]["batches"]["8"]["launches"]) > len(golden["default/graph"]["batches"]["8"]["launches"])


@pytest.mark.parametrize("program", list(lg.PROGRAMS))
def test_stage_profile_records_one_mark_per_stage(models, golden, program):
    """wz_profile_stages refuses a batch whose enqueue did not record exactly one mark per stage name ("%zu marks for %zu stages"):
    it succeeds at batch 1 and 8, and names the stages as recorded."""
    e = HipEngine(models[program], 0, lg.MAX_BATCH, 640, 480, dev=True)
    try:
        assert e.stage_names() == golden[program + "/graph"]["stages"]
        d = [e.upload(synthetic_frame(640, 480, lg.FRAME_SEED + i)) for i in range(lg.MAX_BATCH)]
        for n in (1, 8):
            stages = e.profile_device(d[:n], [640] * n, [480] * n, reps=1)
            assert [s for s, _ in stages] == e.stage_names()
            assert all(np.isfinite(ms) and ms >= 0 for _, ms in stages)
    finally:
        e.close()
