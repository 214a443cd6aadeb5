"""Generates tests/golden/reference_layout.json from a checkout of the reference Watsor sources:
the memory layout of its shared-memory structs (`watsor/stream/share.py:11-32`), its COCO label table
(`watsor/config/coco.py`) and the verdicts of its own ConfidenceFilter / AreaFilter on seeded detections
(the config of tests/golden/filters.json).  tests/test_abi.py and tests/test_filters_oracle.py hold the
package against this record, so they need no copy of the reference at test time.

    python tests/golden/make_reference_golden.py <path of a Watsor checkout>
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def layout(struct):
    """sizeof + (name, ctypes type name, offset, size) of every field."""
    return dict(size=ctypes.sizeof(struct),
                fields=[[name, ftype.__name__, getattr(struct, name).offset, getattr(struct, name).size]
                        for name, ftype in struct._fields_])


def filter_cases(config, confidence_filter, area_filter, detection, bounding_box):
    """The seeded detections of test_coco_table_and_filters_against_reference and the reference's verdicts on them."""
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(300):
        x0, y0 = int(rng.integers(0, 600)), int(rng.integers(0, 440))
        label, score = int(rng.choice([0, 1, 3, 8, 5])), float(np.float32(rng.random()))
        box = [x0, y0, int(rng.integers(x0, 640)), int(rng.integers(y0, 480))]
        d = detection(label=label, confidence=score, bounding_box=bounding_box(*box))
        cases.append(dict(label=label, confidence=score, box=box,
                          conf_pass=bool(confidence_filter(d)), area_pass=bool(area_filter(d))))
    return cases


def main(reference):
    sys.path.insert(0, reference)
    from watsor.config.coco import COCO_CLASSES
    from watsor.filter.area import AreaFilter
    from watsor.filter.confidence import ConfidenceFilter
    from watsor.stream import share
    config = json.load(open(os.path.join(HERE, "filters.json")))["config"]
    out = dict(structs={name: layout(getattr(share, name)) for name in ("BoundingBox", "Detection", "Header")},
               coco_classes=list(COCO_CLASSES),
               filter_cases=filter_cases(config, ConfidenceFilter(config), AreaFilter(config), share.Detection, share.BoundingBox))
    json.dump(out, open(os.path.join(HERE, "reference_layout.json"), "w"))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
