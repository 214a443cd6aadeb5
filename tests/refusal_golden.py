"""The refusals of the tiled, gated, motion and frame-table entry points, pinned verbatim: every case of the refusal tables of
test_gpu_tiled.py, test_gpu_gated.py, test_gpu_bound_tiles.py and test_gpu_motion.py compares its (return code, wz_last_error text) with
tests/golden/tile_refusals.json, which tests/golden/make_tile_refusals_golden.py records by running those four tests."""
import json
import os

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_refusals.json")
RECORD = None          # the recorder puts a dict here: `check` then fills it instead of comparing
_golden = None


def check(table, case, rc, text):
    """case `case` of table `table` returned `rc` and left `text`: what the recording says (both `-p 16` programs say the same)"""
    global _golden
    key, got = "%s/%s" % (table, case), [int(rc), str(text)]
    if RECORD is not None:
        assert RECORD.setdefault(key, got) == got, (key, RECORD[key], got)
        return
    if _golden is None:
        with open(PATH) as f:
            _golden = json.load(f)
    assert key in _golden, "%s is not in %s: record it again" % (key, PATH)
    assert got == _golden[key], (key, got, _golden[key])
