"""Generates tests/golden/tile_refusals.json: the (return code, wz_last_error text) of every case in the refusal tables of
tests/test_gpu_tiled.py, tests/test_gpu_gated.py, tests/test_gpu_bound_tiles.py and tests/test_gpu_motion.py, as the library built from the tree says them.

Needs the GPU (a refusal is checked on a live engine):   python tests/golden/make_tile_refusals_golden.py
It runs those four tests with tests/refusal_golden.py recording instead of comparing, so the tables exist once -- in the tests.
Record on the commit whose texts are to be kept, i.e. BEFORE a change that must not alter them.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import refusal_golden                                        # noqa: E402

TABLES = ["test_gpu_tiled.py::test_refusals_write_nothing_and_leave_the_engine_usable",
          "test_gpu_gated.py::test_refusals_write_nothing_and_keep_the_state",
          "test_gpu_bound_tiles.py::test_refusals_name_the_numbers_and_change_nothing",
          "test_gpu_motion.py::test_refusals_write_nothing_and_keep_the_state"]


def main():
    refusal_golden.RECORD = {}
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(TESTS, t) for t in TABLES])
    if rc != 0:
        sys.exit("the refusal tests did not pass (pytest: %d): nothing written" % rc)
    with open(refusal_golden.PATH, "w") as f:
        json.dump(refusal_golden.RECORD, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)" % (refusal_golden.PATH, len(refusal_golden.RECORD)))


if __name__ == "__main__":
    main()
