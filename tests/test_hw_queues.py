"""GPU_MAX_HW_QUEUES after the library loaded (include/watsor_hip.h: wz_hw_queues; no GPU needed): four lanes need a hardware queue each
beside the runtime's own, so whatever the host pinned below 8 -- nothing, an empty string, not a number, 1, 4 -- becomes 8, and a host
that chose 8 or more keeps its choice.  Fresh child processes: the variable is written by a load-time constructor, into the C
environment (which `os.environ` does not see)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
VAR = "GPU_MAX_HW_QUEUES"

CHILD = ("import ctypes, sys; sys.path.insert(0, %r)\n"
         "from watsor_amd import _lib, runtime\n"
         "libc = ctypes.CDLL(None); libc.getenv.restype = ctypes.c_char_p; libc.getenv.argtypes = [ctypes.c_char_p]\n"
         "before = libc.getenv(b'" + VAR + "')\n"
         "dev = sys.argv[1] == 'dev'\n"
         "lib = _lib.load(dev=dev)\n"
         "after = libc.getenv(b'" + VAR + "')\n"
         "print('before=%%r after=%%r lib=%%d wrapper=%%d' %% (before, after, lib.wz_hw_queues(), runtime.hw_queues(dev=dev)))\n") % ROOT

# (what the host set, what the process runs on)
CASES = [(None, 8), ("", 8), ("abc", 8), ("1", 8), ("4", 8), ("8", 8), ("16", 16), ("32", 32)]


@pytest.mark.parametrize("library", ["product", "dev"])
@pytest.mark.parametrize("given,expected", CASES, ids=["unset" if g is None else "%r" % g for g, _ in CASES])
def test_library_takes_eight_queues_and_keeps_a_larger_choice(given, expected, library):
    env = {k: v for k, v in os.environ.items() if k != VAR}
    if given is not None:
        env[VAR] = given
    p = subprocess.run([sys.executable, "-c", CHILD, library], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    before = "None" if given is None else repr(given.encode())
    # the value is left byte for byte where the host's choice stands ("16" stays "16"), and is exactly "8" where it did not
    assert p.stdout.strip() == "before=%s after=%r lib=%d wrapper=%d" % (before, str(expected).encode(), expected, expected), p.stdout + p.stderr


WARN_CHILD = ("import ctypes, logging, os, sys, tempfile; sys.path.insert(0, %r)\n"
              "from watsor_amd import _lib\n"
              "from watsor_amd.detection import hip_gpu\n"
              "_lib.load()\n"
              "if sys.argv[1] != 'keep':\n"
              "    ctypes.CDLL(None).setenv(b'" + VAR + "', sys.argv[1].encode(), 1)      # changed after the library loaded\n"
              "class Engine:\n"
              "    def __init__(self, *a, **k): pass\n"
              "hip_gpu.HipEngine = Engine\n"
              "seen = []\n"
              "class Keep(logging.Handler):\n"
              "    def emit(self, record): seen.append(record.getMessage())\n"
              "logging.getLogger(hip_gpu.__name__).addHandler(Keep(level=logging.WARNING))\n"
              "d = tempfile.mkdtemp(); open(os.path.join(d, hip_gpu.ENGINE_FILE), 'wb').write(b'stub')\n"
              "for _ in range(2):\n"
              "    hip_gpu.HipObjectDetector(d, 0, {'numa': False})\n"
              "print(len(seen), seen[0] if seen else '')\n") % ROOT


@pytest.mark.parametrize("after_load,lanes,warnings", [("keep", None, 0), ("4", None, 1), ("7", None, 1), ("8", None, 0), ("8", "5", 1), ("4", "2", 0)])
def test_detector_warns_once_below_two_queues_per_lane(after_load, lanes, warnings):
    """The plugin's one warning per process (watsor_amd/detection/hip_gpu.py): the variable below 2 x the lanes wz_create will make (WZ_LANES,
    else 4) -- here because it was changed after the library loaded.  The engine is a stub: no GPU."""
    env = {k: v for k, v in os.environ.items() if k not in (VAR, "WZ_LANES")}
    if lanes is not None:
        env["WZ_LANES"] = lanes
    p = subprocess.run([sys.executable, "-c", WARN_CHILD, after_load], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    count, _, message = p.stdout.strip().partition(" ")
    assert int(count) == warnings, p.stdout + p.stderr
    if warnings:
        assert VAR in message and "hardware queues" in message, message
