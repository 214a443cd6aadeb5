"""The plugin option `tiles` with a `gate` (watsor_amd/detection/hip_gpu.py: tile_options; no GPU needed)."""
import pytest

from watsor_amd.detection.hip_gpu import tile_options

RECTS = [[0, 0, 64, 48], [32, 16, 64, 48]]


def test_gate_is_accepted_with_defaults():
    spec, by_name = tile_options({"tiles": {"rects": RECTS, "gate": {"threshold": 8}}})
    assert spec["gate"] == (8, 1, 0) and spec["count"] == 2 and not by_name
    spec, _ = tile_options({"tiles": {"grid": [2, 2], "overlap": 0.2, "ios": 0.6, "gate": {"threshold": 0, "min_cells": 3, "max_age": 25}}})
    assert spec["gate"] == (0, 3, 25) and spec["ios"] == 0.6 and spec["count"] == 5
    spec, _ = tile_options({"tiles": {"rects": RECTS, "gate": {"threshold": 255}}})
    assert spec["gate"] == (255, 1, 0)
    _, by_name = tile_options({"tiles": {"porch": {"rects": RECTS, "gate": {"threshold": 4}}, "yard": {"rects": RECTS}}})
    assert by_name["porch"]["gate"] == (4, 1, 0) and "gate" not in by_name["yard"]
    spec, _ = tile_options({"tiles": {"rects": RECTS}})
    assert "gate" not in spec


@pytest.mark.parametrize("gate", [
    8, "8", [8], None, True, {},                                                 # not a description / no threshold
    {"threshold": 8.0}, {"threshold": "8"}, {"threshold": True}, {"threshold": None},
    {"threshold": -1}, {"threshold": 256},
    {"threshold": 8, "min_cells": 0}, {"threshold": 8, "min_cells": -2}, {"threshold": 8, "min_cells": 1.5},
    {"threshold": 8, "max_age": -1}, {"threshold": 8, "max_age": "2"},
    {"threshold": 8, "cells": 1}, {"threshold": 8, "min_cells": 1, "max_age": 0, "pixel_thr": 3},
])
def test_bad_gates_are_refused(gate):
    with pytest.raises(ValueError, match="gate"):
        tile_options({"tiles": {"rects": RECTS, "gate": gate}})
    with pytest.raises(ValueError, match="porch"):
        tile_options({"tiles": {"porch": {"grid": [2, 1], "gate": gate}}})


def test_unknown_keys_beside_gate_are_still_refused():
    with pytest.raises(ValueError, match="gates"):
        tile_options({"tiles": {"rects": RECTS, "gates": {"threshold": 8}}})
