"""Shared buffers, every lane, after other batches: the head outputs bit for bit.

The op-by-op conformance runs on engines that keep every tensor in a buffer of its own, sized for the batch, fresh, on lane 0.
Production packs tensors into slots by liveness (engine.assign_slots; tests/test_slot_liveness_cpu.py replays the rule on the CPU),
sizes slots and workspace for max_batch, and runs batches of any size on four lanes one after the other.  Here, for every program of
launch_golden.PROGRAMS (without the twelve-head one), two development engines of max_batch 9 in one process, one with kept and one
with shared buffers (tests/production_batches.py: child_bits):
  * both first run the network at n = 9 on an all-NaN input (stage_forward: no post-processing): lane 0's tensors, slots and
    workspace hold what the engine's largest batch left of it.  On the MI355X that is NaN only up to the first ReLU6 -- the clamp
    returns its bound for a NaN -- and saturated, finite values behind it: stale data of a larger batch in every slot and in the
    workspace, not NaN everywhere (the share of NaN among that pass's logits is printed, not asserted: measured 0);
  * the kept engine runs detect_batch on batches of 8, 3, 9, 1, 5, 2, 6 frames, twice each: the same box encodings and class logits
    as uint32, all finite;
  * the shared engine runs the same batches on lanes 0, 1, 2, 3, 0, 1, 2 with submit_host + collect -- first the first four with
    all four lanes in flight before the first collect, then the seven one at a time -- and stage_post_lane(lane, n) must equal the
    kept engine's words.
Captured graphs (WZ_GRAPH=1).  For the default and the robust program the same in a second child kernel by kernel (WZ_GRAPH=0,
`lone` set), whose head outputs at n = 3, 5 and 8 -- and every other size of the sequence -- must be the captured graphs': the two
shapes of launch A of blocks 13 .. 16 (k_mbconv_hp2.hip) compute bit-identical tensors.

The test does not compare constants: in every batch any two frames' logits differ, and no two batches begin with the same logits."""
import pytest

import launch_golden as lg
import production_batches as pb

pytestmark = pytest.mark.gpu

PROGRAMS = [p for p in lg.PROGRAMS if p != "heads_twice"]
_results = {}


def _run(program, env, tmp_path_factory):
    if (program, env) not in _results:
        _results[(program, env)] = pb.run_child(dict(mode="bits", program=program), env,
                                                tmp_path_factory.mktemp("bits_%s_%s" % (program, env)), timeout=180)
    p, out = _results[(program, env)]                     # (a child that failed is not started a second time)
    assert out is not None, "child exited with %s:\n%s" % (p.returncode, p.stderr[-3000:])
    return out


def _check(out, env, what):
    assert out["slots"][0] < out["slots"][1], "%s: %d slots for %d tensors: nothing is shared" % ((what,) + tuple(out["slots"]))
    print("\n%s: %d slots for %d tensors; NaN among the logits of the poisoning pass: kept %.3f, shared %.3f"
          % ((what,) + tuple(out["slots"]) + tuple(out["poison_nan"])))
    assert [(b["n"], b["lane"]) for b in out["batches"]] == list(pb.SEQUENCE)
    assert out["messages"] == [], "%s:\n  %s" % (what, "\n  ".join(out["messages"]))
    for b in out["batches"]:
        assert b["finite"] and b["kept_repeats"] and b["shared_equals_kept"], (what, b)
        assert b["frames_differ"], (what, b)
        assert (b["shared_graph_nodes"] > 0) == (env == "graph") and (b["kept_graph_nodes"] > 0) == (env == "graph"), (what, b)
    assert out["batches_differ"], what
    assert [(b["n"], b["lane"]) for b in out["four_lanes"]] == list(pb.SEQUENCE[:4]) and all(b["equal"] for b in out["four_lanes"]), what
    assert all((b["graph_nodes"] > 0) == (env == "graph") for b in out["four_lanes"]), what


@pytest.mark.parametrize("program", PROGRAMS)
def test_shared_buffers_any_lane_after_other_batches(tmp_path_factory, program):
    _check(_run(program, "graph", tmp_path_factory), "graph", program)


@pytest.mark.parametrize("program", lg.KNOB_PROGRAMS)
def test_kernel_by_kernel_heads_equal_the_captured_graphs(tmp_path_factory, program):
    lone = _run(program, "kernel_by_kernel", tmp_path_factory)
    _check(lone, "kernel_by_kernel", program + ", kernel by kernel")
    graph = _run(program, "graph", tmp_path_factory)
    assert {3, 5, 8} <= {b["n"] for b in lone["batches"]}
    for a, b in zip(lone["batches"], graph["batches"]):
        assert a["n"] == b["n"] and a["sha256"] == b["sha256"], "%s: batch of %d frames: kernel by kernel and captured graph differ" % (program, a["n"])
