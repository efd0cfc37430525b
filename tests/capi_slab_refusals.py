"""The one run of tests/capi_slab_refusals_worker.py that the test_c_api_refuses_an_object_on_several_slabs tests of the six mesh
parts share: started by the first of them that asks, kept for the session."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_run = None


def refusal(launcher, part):
    """What launcher.run returned for the worker - MC33_HIP_DEVICES=0,0 in a fresh process, before the library is loaded: two slabs
    on one device - with stdout cut down to the line of `part` (measure, topology, filter, smooth, simplify, clip)."""
    global _run
    if _run is None:
        _run = launcher.run([sys.executable, os.path.join(HERE, "capi_slab_refusals_worker.py")], env={"MC33_HIP_DEVICES": "0,0"}, timeout=300)
    lines = [x for x in _run["stdout"].splitlines() if x.startswith(part + " refused: ")]
    return dict(_run, stdout="\n".join(lines), all_stdout=_run["stdout"])
