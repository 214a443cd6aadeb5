"""SSD-Inception-v2 engines on the MI355X (watsor_amd/inception.py, csrc/k_inception.hip): every tensor against the CPU oracle of
tests/inception_v2_oracle.py, the scores, the plugin end to end, the asynchronous / bound / graph-replayed paths, and a MobileNet-v2
engine beside an Inception one in the same process.

Tolerances: `-p 32` agrees with the fp32 oracle to fp32 rounding (tensors 1e-4 of their range, scores 1e-4); `-p 16` keeps the plain
fp16 programs' LOGIT_TOL / BOXENC_TOL of tests/test_gpu_parity.py on the heads and 1e-3 on the scores (the CPU emulation of this
program: 3.2e-4, profiles/inception_fp16_emulation.json)."""
import os

import numpy as np
import pytest

import conftest
import parity_utils as pu
from inception_v2_oracle import InceptionOracleDetector, InceptionOracleNet
from oracle import detect as odet
from oracle.compare import assert_rows_match
from oracle.postprocess import sigmoid
from watsor_amd import engine
from watsor_amd.runtime import FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.05        # tests/test_gpu_parity.py: the plain fp16 programs against the fp32 oracle
BOXENC_TOL = 0.04
SCORE_TOL = 1e-3
SEED = 1234


@pytest.fixture(scope="module")
def inc_weights():
    return synthetic_inception_v2(SEED)


@pytest.fixture(scope="module")
def inc_dirs(tmp_path_factory, inc_weights):
    out = {}
    for p in (16, 32):
        d = tmp_path_factory.mktemp("inception_p%d" % p)
        engine.save_engine(engine.build_engine(inc_weights, p), os.path.join(str(d), "mi355x.bin"))
        out[p] = str(d)
    return out


@pytest.fixture(scope="module")
def frames():
    return [synthetic_frame(640, 480, 5000 + i) for i in range(2)]


@pytest.fixture(scope="module")
def oracle_out(inc_weights, frames):
    x_half = pu.oracle_input_half(frames)
    be, lg, T = pu.oracle_forward_from_half(InceptionOracleNet(inc_weights), x_half, keep=True)
    return x_half, be, lg, T


def _keep_engine(path):
    os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        return conftest.make_engine(path, max_batch=2, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE")


@pytest.mark.parametrize("precision", [32, 16])
def test_every_tensor_close_to_oracle(inc_dirs, oracle_out, precision):
    x_half, rbe, rlg, T = oracle_out
    e = _keep_engine(inc_dirs[precision])
    try:
        be, lg = e.stage_forward(x_half)
        worst = {}
        for idx, (name, h, w, c) in enumerate(e.tensors()):
            if name == "input":
                continue
            got = np.stack([e.stage_read_tensor(idx, f) for f in range(2)]).astype(np.float32)
            if name not in T:                 # branch intermediates: the oracle keeps module outputs and trunk tensors; each of the 38
                continue                      # is checked on its own, against its op's float64 reference, in tests/test_gpu_op_conformance.py
            ref = T[name]
            assert got.shape == ref.shape, name
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            bound = (1e-4 * scale + 1e-5) if precision == 32 else (0.04 * scale + 0.02)
            assert err <= bound, "%s (-p %d): max abs err %.3g (max|ref| %.3f)" % (name, precision, err, scale)
            worst[name] = err / max(scale, 1e-12)
        for name in ("Conv2d_1a_7x7", "MaxPool_2a_3x3", "Mixed_3b", "Mixed_4a", "Mixed_4c", "Mixed_5a", "Mixed_5c"):
            assert name in worst, name
        print("\n-p %d: worst relative tensor error %.2e (%s)" % (precision, max(worst.values()), max(worst, key=worst.get)))
        tol_b, tol_l = (1e-3, 1e-3) if precision == 32 else (BOXENC_TOL, LOGIT_TOL)
        assert np.abs(be - rbe).max() <= tol_b and np.abs(lg - rlg).max() <= tol_l
        dscore = float(np.abs(sigmoid(lg) - sigmoid(rlg)).max())
        print("-p %d: max |dscore| over all 1917 x 91 entries: %.2e" % (precision, dscore))
        assert dscore <= (1e-4 if precision == 32 else SCORE_TOL)
    finally:
        e.close()


@pytest.mark.parametrize("precision", [16, 32])
def test_detect_end_to_end_matches_oracle_detector(inc_dirs, inc_weights, precision):
    """Rows through the plugin class against the oracle detector on 640x480, 1280x720 and 1920x1080 frames."""
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    oracle = InceptionOracleDetector(inc_weights)
    frames = [synthetic_frame(640, 480, 6000), synthetic_frame(1280, 720, 6001), synthetic_frame(1920, 1080, 6002)]
    with HipObjectDetector(inc_dirs[precision], 0) as det:
        for f in frames:
            rows = DetectionArray()
            assert det.detect(f.shape, f, rows) > 0
            got = np.frombuffer(rows, dtype=ROW_DTYPE)
            b, c, s, _, _ = oracle.raw(f)
            r = assert_rows_match(got, odet.rows_as_array(f.shape, b, c, s), f.shape, tol=SCORE_TOL,
                                  what="-p %d %dx%d" % (precision, f.shape[1], f.shape[0]))
            assert len(r["pairs"]) >= 90


@pytest.fixture(scope="module")
def batch_frames():
    sizes = [(640, 480), (1280, 720), (1920, 1080), (640, 480)]
    return [synthetic_frame(w, h, 7000 + i) for i, (w, h) in enumerate(sizes * 4)]   # 16 frames, mixed sizes


@pytest.mark.parametrize("n", [1, 8, 16])
def test_batches_match_oracle(inc_dirs, inc_weights, batch_frames, n):
    """detect_batch at batch 1, 8 and 16 (mixed frame sizes) against the oracle detector, frame by frame."""
    oracle = InceptionOracleDetector(inc_weights)
    e = conftest.make_engine(inc_dirs[16], max_batch=16)
    try:
        fr = batch_frames[:n]
        rows = [np.zeros(100, ROW_DTYPE) for _ in fr]
        e.detect_batch(fr, rows)
        for f, got in zip(fr[:4], rows[:4]):
            b, c, s, _, _ = oracle.raw(f)
            assert_rows_match(got, odet.rows_as_array(f.shape, b, c, s), f.shape, tol=SCORE_TOL, what="batch %d" % n)
    finally:
        e.close()


def test_host_bound_and_replayed_paths_equal_detect_batch(inc_dirs, batch_frames):
    """wz_submit_host + wz_collect and the bound-frame path give the rows of wz_detect_batch bit for bit, with all lanes busy
    (graph replay) as well as one batch at a time (kernel by kernel)."""
    e = conftest.make_engine(inc_dirs[16], max_batch=8)
    try:
        batches = [batch_frames[0:3], batch_frames[3:8], batch_frames[8:9], batch_frames[9:13]]
        refs = []
        for b in batches:
            ref = [np.zeros(100, ROW_DTYPE) for _ in b]
            e.detect_batch(b, ref)
            refs.append(ref)
        assert e.num_slots >= len(batches)
        for rep in range(2):                   # the second round replays the graphs captured in the first
            for lane, b in enumerate(batches):
                e.submit_host(lane, b)
            for lane, b in enumerate(batches):
                got = [np.zeros(100, ROW_DTYPE) for _ in b]
                e.collect(lane, got)
                for g, r in zip(got, refs[lane]):
                    assert g.tobytes() == r.tobytes(), (rep, lane)
        flat = [f for b in batches for f in b]
        rows = np.zeros((len(flat), 100), ROW_DTYPE)
        e.bind_frames([f.ctypes.data for f in flat], [f.shape[1] for f in flat], [f.shape[0] for f in flat], [FMT_RGB24] * len(flat),
                      [-1] * len(flat), [rows[i].ctypes.data for i in range(len(flat))])
        entries, k = [], 0
        for b in batches:
            entries.append(list(range(k, k + len(b))))
            k += len(b)
        for lane, ent in enumerate(entries):
            e.submit_bound(lane, ent)
        for lane, ent in enumerate(entries):
            e.collect_bound(lane)
            for j, i in enumerate(ent):
                assert rows[i].tobytes() == refs[lane][j].tobytes(), (lane, j)
        e.bind_frames([], [], [], [], [], [])
    finally:
        e.close()


def test_mobilenet_and_inception_engines_in_one_process(model_dir, synth_weights, inc_dirs, inc_weights):
    """Two networks open at once: each engine gives its own network's rows."""
    f = synthetic_frame(640, 480, 8000)
    e_mb = conftest.make_engine(model_dir, max_batch=2)
    e_in = conftest.make_engine(inc_dirs[16], max_batch=2)
    try:
        for _ in range(2):
            for e, oracle in ((e_mb, odet.OracleObjectDetector(weights=synth_weights)), (e_in, InceptionOracleDetector(inc_weights))):
                got = np.zeros(100, ROW_DTYPE)
                e.detect_batch([f], [got])
                b, c, s, _, _ = oracle.raw(f)
                assert_rows_match(got, odet.rows_as_array(f.shape, b, c, s), f.shape, tol=SCORE_TOL)
    finally:
        e_in.close()
        e_mb.close()
