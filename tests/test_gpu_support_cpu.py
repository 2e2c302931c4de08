"""The child-process runner of tests/gpu_support.py without a GPU: a child that outlives its time limit is ended
with everything it started, and a child that fails fails the test with its stderr."""
import os
import sys
import time

import pytest

from tests.gpu_support import child_env, run_command

# starts a sleeping child of its own, prints both pids (to stdout and, since a child that times out returns
# nothing, to the file named by its argument), then sleeps too
_PARENT = """import os, subprocess, sys, time
g = subprocess.Popen([sys.executable, "-c", "import time; time.sleep(600)"])
for f in (sys.stdout, open(sys.argv[1], "w")):
    print(os.getpid(), g.pid, file=f, flush=True)
time.sleep(600)
"""


def _gone(pid, within=5.0):
    """os.kill(pid, 0) raises ProcessLookupError, now or within `within` seconds."""
    end = time.time() + within
    while True:
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            return True
        if time.time() > end:
            return False
        time.sleep(0.05)


def test_time_limit_ends_the_child_and_what_it_started(tmp_path):
    pidfile = tmp_path / "pids.txt"
    with pytest.raises(pytest.fail.Exception, match="timed out after 1 s"):
        run_command([sys.executable, "-c", _PARENT, str(pidfile)], tmp_path, 1, child_env())
    pids = [int(v) for v in pidfile.read_text().split()]
    assert len(pids) == 2 and pids[0] != pids[1]
    assert all(_gone(pid) for pid in pids)


def test_a_failing_child_fails_the_assertion_with_its_stderr(tmp_path):
    code = "import sys; sys.stderr.write('the reason it failed\\n'); sys.exit(3)"
    with pytest.raises(AssertionError, match="the reason it failed"):
        run_command([sys.executable, "-c", code], tmp_path, 60, child_env())
