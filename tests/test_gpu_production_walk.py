"""The op-by-op float64 conformance (tests/op_reference.py: `walk`) on what PRODUCTION ran: not stage_forward on a prepared input, but
detect_batch of n frames of mixed sizes on an engine of max_batch 9 -- the resize kernel fills the input tensor (a pair input with
its lo half, which stage_forward leaves zero), the batch is a captured graph (WZ_GRAPH=1) or goes kernel by kernel with `lone` set
(WZ_GRAPH=0: launch A of the robust program's blocks 13 .. 16 then takes its two-waves-per-chunk form up to 128 workgroups -- block 13
at n = 3 .. 5, blocks 14 .. 16 at n = 5 .. 8), the post-processing runs behind it.  With WZ_NO_BUFFER_REUSE=1 lane 0's tensors stay
readable afterwards and stage_post_lane(0, n) returns the head outputs: the walker checks every op on them, with its own bounds and
its own coverage asserts (tests/production_batches.py: the programs, the cases, the frames and the child process of each
environment, which runs its cases one after the other).

Besides the walk, per batch:
  * the stored input tensor of EVERY frame equals oracle.preprocess bit for bit, hi and lo (the resize inside a batch of mixed sizes);
  * a pair input's lo half is populated: non-zero in at least 90 % of each frame's R, G, B elements -- a condition on the test's
    input, so that "the first op reads lo" is checked on data where lo exists (the first op's reference is built from the stored
    halves summed in float64);
  * graph_nodes(0) is 0 kernel by kernel and positive for a captured graph; decode_fused and cands_listed are what
    tests/golden/network_launches.json records for the program (the recording does not hold the Inception-v2 and MobileNet-v1
    `-p 32` programs: UNRECORDED_FLAGS says what is expected of them and why)."""
import pytest

import launch_golden as lg
import production_batches as pb

pytestmark = pytest.mark.gpu


# The Inception-v2 and MobileNet-v1 `-p 32` programs are not in the recording.  Their six heads are the [box | class] heads of the
# `-p 16` programs of the same families, which the recording holds with both flags set at every batch size, and enqueue_conv_f32 parks
# a head's partial sums by the same rule (HeadPark::slab) whenever its K is split: every head in the grouped reduce, which then decodes
# and lists -- as the MobileNet-v2 `-p 32` program is recorded.  A head that stopped parking would clear both flags.
UNRECORDED_FLAGS = (True, True)


@pytest.fixture(scope="module")
def golden():
    return lg.golden()


@pytest.fixture(scope="module")
def workers(tmp_path_factory):
    """environment -> its child process (production_batches.Worker), started on first use"""
    made = {}

    def get(env):
        if env not in made:
            made[env] = pb.Worker(env, tmp_path_factory.mktemp("walk_" + env))
        return made[env]
    yield get
    for w in made.values():
        w.close()


@pytest.mark.parametrize("program,env,n", pb.WALK_CASES, ids=["%s-%s-b%d" % c for c in pb.WALK_CASES])
def test_every_op_of_a_production_batch_within_its_own_bound(golden, workers, tmp_path, program, env, n):
    n_blocks, key = pb.WALK_PROGRAMS[program][3], pb.WALK_PROGRAMS[program][5]
    out = workers(env).run(dict(mode="walk", program=program, batches=[n]), tmp_path, timeout=120)
    # which programs have a pair input is part of what is tested: the stem-separate program has none
    assert out["input_pair"] == (program in pb.PAIR_INPUT)
    assert out["blocks"] == n_blocks
    if key is None:
        flags = UNRECORDED_FLAGS
    else:
        recorded = {(b["decode_fused"], b["cands_listed"]) for b in golden["%s/%s" % (key, env)]["batches"].values()}
        assert len(recorded) == 1
        flags = recorded.pop()
    assert sorted(out["batches"]) == [str(n)]
    for b in out["batches"].values():
        print("\n%s, %s, batch %d (%s): %s\n  resize + batch %.2f s, walk %.2f s; graph nodes %d; lo half non-zero per frame: %s"
              % (program, env, n, " ".join(b["sizes"]), b["summary"], b["seconds_batch"], b["seconds_walk"], b["graph_nodes"],
                 " ".join("%.4f" % v for v in b["lo_populated"]) or "(no pair input)"))
        what = "%s, %s, batch %d" % (program, env, n)
        assert b["input_differs"] == [], what
        if out["input_pair"]:
            assert len(b["lo_populated"]) == n and min(b["lo_populated"]) >= pb.LO_POPULATED, what
        else:
            assert b["lo_populated"] == []
        assert (b["graph_nodes"] == 0) if env == "kernel_by_kernel" else (b["graph_nodes"] > 0), what
        assert (b["decode_fused"], b["cands_listed"]) == flags, what
        assert b["n_failures"] == 0, "%s: %d failure(s):\n  %s" % (what, b["n_failures"], "\n  ".join(b["failures"]))
        assert b["ops_mbconv"] == 0 and b["blocks_checked"] == n_blocks and b["ops_unchecked"] == 0 and b["ops_checked"] == out["ops"]
        assert b["elements"] > 0 and b["worst"] <= 1.0
