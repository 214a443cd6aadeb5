"""Both resize kernels swept over the case list of tests/resize_cases.py: every row count R = 1 .. 8 of the row-staged kernel, its
divisor and tail cases, one, two and three trips of its staging loop, the scale-2 switch, every residue of its runs' alignment, the
60 KiB switch-off, tiny and lopsided frames, both coordinate rules on every format, and the per-pixel kernel's byte-wise tails
(what the list covers is asserted on the CPU, tests/test_resize_cases_cpu.py).

The reference for every stored value is oracle/preprocess.py on the RGB bytes tests/pixfmt_oracle.py / tests/pixfmt10_oracle.py work
out of the frame -- never the GPU's own RGB24 path --, bit for bit: the hi half, the lo half, and zeros in the fourth channel.
tests/resize_plan.py says which class a case runs, and each test asserts that before it compares."""
import os

import numpy as np
import pytest

import resize_cases as rc
import resize_plan as rp
import test_gpu_pixfmt as eight
import test_gpu_variants as variants
from watsor_amd.runtime import ROW_DTYPE

pytestmark = pytest.mark.gpu

KERNELS = ("pixel", "rows")
RULE_NAMES = {False: "legacy", True: "half_pixel"}


class Engines:
    """Development engines by (class of tests/resize_cases.ENGINES, kernel form, coordinate rule), made at first use and kept to the
    end of the module; all of them keep every tensor in a buffer of its own (WZ_NO_BUFFER_REUSE=1), so that a batch's stored input
    can be read back after the network has run."""

    def __init__(self, dirs):
        self.dirs, self.made = dirs, {}

    def get(self, cls, kernel, half_pixel):
        key = (cls, kernel, half_pixel)
        if key not in self.made:
            max_w, max_h, max_batch = rc.ENGINES[cls]
            saved = os.environ.get("WZ_NO_BUFFER_REUSE")
            os.environ["WZ_NO_BUFFER_REUSE"] = "1"
            try:
                self.made[key] = eight.engine_with(self.dirs[half_pixel], {"WZ_PRE_ROWS": "1" if kernel == "rows" else "0"},
                                                   max_batch=max_batch, max_width=max_w, max_height=max_h)
            finally:
                os.environ.pop("WZ_NO_BUFFER_REUSE")
                if saved is not None:
                    os.environ["WZ_NO_BUFFER_REUSE"] = saved
        return self.made[key]

    def close(self):
        for e in self.made.values():
            e.close()


@pytest.fixture(scope="module")
def engines(model_dir_default, tmp_path_factory, synth_weights):
    e = Engines({False: model_dir_default, True: variants.build(tmp_path_factory, synth_weights, "half_pixel_sweep", resize="half_pixel")})
    yield e
    e.close()


def assert_stored_input(hi, lo, fourth, fmt, w, h, half_pixel, what):
    """hi, lo: float16 [300, 300, 3] as stored; fourth: whatever the fourth channels hold"""
    want_hi, want_lo = rc.stored_input(fmt, w, h, half_pixel)
    for name, got, want in (("hi", hi, want_hi), ("lo", lo, want_lo)):
        got, want = np.ascontiguousarray(got).view(np.uint16), want.view(np.uint16)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("%s: %d %s halves differ from the oracle, the first at (row, column, channel) %s: 0x%04x, expected 0x%04x; "
                                 "rows %d .. %d" % (what, len(bad), name, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])],
                                                    bad[:, 0].min(), bad[:, 0].max()))
    assert not np.ascontiguousarray(fourth).view(np.uint16).any(), what + ": the fourth channel is not zero"


def runs_rows_kernel(c, kernel):
    """the host's rule (wz_engine.hip: read_options, rows_fit) for a case on its engine"""
    max_w = rc.ENGINES[c.engine][0]
    return kernel == "rows" and rp.engine_keeps_rows_kernel(max_w) and rp.rows_fit(c.w, c.fmt, rp.wz_preprocess_rows_lds(max_w))


SWEEP = [(c, hp, k) for c in rc.CASES if c.engine in ("std", "wide") for hp in (False, True) for k in KERNELS]


@pytest.mark.parametrize("case,half_pixel,kernel", SWEEP, ids=["%s-%s-%s" % (rc.case_id(c), RULE_NAMES[hp], k) for c, hp, k in SWEEP])
def test_stored_input_equals_the_oracle(engines, case, half_pixel, kernel):
    c = case
    if kernel == "rows":                                            # the class the list claims is the class the plan says this launch runs
        assert runs_rows_kernel(c, kernel)
        p = rc.case_plan(c, half_pixel)                             # (lane 0's staging area is its own allocation: address residue 0)
        assert (p.R, p.workgroups[-1].nrows, rp.trips(p)) == rc.listed(c, half_pixel)
        assert rp.lds_used(p) <= p.budget == rc.budget(c.engine)
    eng = engines.get(c.engine, kernel, half_pixel)
    assert eng.tensor_is_pair(0)
    got = eng.stage_preprocess(rc.frame(c.fmt, c.w, c.h)[0], c.fmt)
    assert got.shape == (rp.SIZE, rp.SIZE, 8)
    assert_stored_input(got[..., 0:3], got[..., 4:7], got[..., [3, 7]], c.fmt, c.w, c.h, half_pixel, rc.case_id(c))


LIMIT = [c for c in rc.CASES if c.engine.startswith("limit")]


@pytest.mark.parametrize("case", LIMIT, ids=[rc.case_id(c) for c in LIMIT])
def test_the_60_kib_limit(engines, case):
    """max_width 6816 is the widest engine whose row-staged launch stays within 60 KiB, and it keeps that kernel -- its widest frame
    fills three trips of the staging loop --; 6817 loses it, and WZ_PRE_ROWS=1 then runs the per-pixel kernel.  Which kernel ran is
    the host's rule restated (the development library reports no launch of a stage call): what is checked on the GPU is that either
    side of the limit stores the oracle's input."""
    c = case
    keeps = c.engine == "limit_keeps"
    assert runs_rows_kernel(c, "rows") == keeps
    assert (rc.budget(c.engine) <= rp.LDS_LIMIT) == keeps
    if keeps:
        p = rc.case_plan(c)
        assert (p.R, p.workgroups[-1].nrows, rp.trips(p)) == rc.listed(c, False) and rp.lds_used(p) <= p.budget
    got = engines.get(c.engine, "rows", False).stage_preprocess(rc.frame(c.fmt, c.w, c.h)[0], c.fmt)
    assert_stored_input(got[..., 0:3], got[..., 4:7], got[..., [3, 7]], c.fmt, c.w, c.h, False, rc.case_id(c))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("half_pixel", [False, True], ids=["legacy", "half_pixel"])
def test_mixed_batches_at_every_device_address_residue(engines, half_pixel, kernel):
    """Two batches of eight frames in ONE launch each -- blockIdx.y > 0, with R = 1, 2, 3, 5, 7 and 8 (and 4, 6) side by side, seven
    formats, and the frames at device addresses of all 16 residues mod 16, RGB24 at 1, 2 and 3 mod 4: after the batch ran, every
    frame's stored input is the oracle's, bit for bit.  The plan is evaluated at the address the frame really has."""
    eng = engines.get("std", kernel, half_pixel)
    for b, batch in enumerate(rc.BATCHES):
        ptrs, at = [], []
        try:
            for f in batch:
                frame = rc.frame(f.fmt, f.w, f.h)[0]
                ptrs.append(eng.upload(np.concatenate([np.full(f.residue, 0xEE, np.uint8), frame.reshape(-1).view(np.uint8), np.full(32, 0xEE, np.uint8)])))
                assert ptrs[-1] % 16 == 0                           # (a device allocation is aligned far beyond 16 bytes)
                at.append(ptrs[-1] + f.residue)
                p = rp.plan(f.w, f.h, f.fmt, rc.budget("std"), half_pixel, at[-1])
                assert p.R == f.R and at[-1] % 16 == f.residue and rp.lds_used(p) <= p.budget
                assert rp.residues(p, 0) == rp.residues(rp.plan(f.w, f.h, f.fmt, rc.budget("std"), half_pixel, f.residue), 0)
            eng.submit_device(0, at, [f.w for f in batch], [f.h for f in batch], formats=[f.fmt for f in batch])
            eng.collect(0, [np.zeros(100, ROW_DTYPE) for _ in batch])
            stored = [eng.stage_read_tensor(0, i, halves=True) for i in range(len(batch))]
        finally:
            eng.sync()
            for p in ptrs:
                eng.free(p)
        for i, (f, (hi, lo)) in enumerate(zip(batch, stored)):
            assert hi.shape == lo.shape == (rp.SIZE, rp.SIZE, 4)
            assert_stored_input(hi[..., :3], lo[..., :3], np.stack([hi[..., 3], lo[..., 3]]), f.fmt, f.w, f.h, half_pixel,
                                "batch %d frame %d (%s %dx%d at residue %d)" % (b, i, rp.NAMES[f.fmt & rp.BASE_MASK], f.w, f.h, f.residue))
