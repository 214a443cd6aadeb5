"""Generates tests/golden/detector_calls.json: what every scenario of tests/detector_calls.py makes the detector plugin
(watsor_amd/detection/hip_gpu.py) ask of the engine -- the calls with their arguments in order, `bound_descriptions`, the returned id
maps and tables, and the type and text of every exception -- under a recording stand-in for `HipEngine`.  No GPU needed:

    python tests/golden/make_detector_calls_golden.py

Record on the commit whose calls are to be kept, i.e. BEFORE a change of the plugin that must not alter them: the script refuses to
write while `git status --porcelain watsor_amd/detection` shows an edit.  The committed file was recorded on a2bd3b7 ("Motion regions
through the worker's frame table"), the parent of the commit that split the option parsing off into watsor_amd/detection/options.py."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import detector_calls as dc                                  # noqa: E402


def main():
    status = subprocess.run(["git", "status", "--porcelain", "watsor_amd/detection"], cwd=ROOT, capture_output=True, text=True)
    if status.returncode != 0 or status.stdout.strip():
        sys.exit("watsor_amd/detection differs from the commit (or git could not say): nothing written\n%s%s" % (status.stdout, status.stderr))
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    from watsor_amd.detection import hip_gpu
    hip_gpu.HipEngine = dc.RecordingEngine
    scenarios = {name: dc.record(name, hip_gpu) for name in dc.SCENARIOS}
    with open(dc.PATH, "w") as f:
        json.dump({"scenarios": scenarios}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d scenarios, %d steps) with watsor_amd/detection as of %s"
          % (dc.PATH, len(scenarios), sum(len(s) for s in scenarios.values()), head))


if __name__ == "__main__":
    main()
