"""What the GPU test files share: the child-process runner, the engine fixtures and the writer of a module's
measured deviations.  A plain module, imported by name (`from tests.gpu_support import eng  # noqa: F401` hands
the importing module a module-scoped fixture of its own)."""
import json
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER_VARS = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")


def child_env(extra_path=None):
    """This process's environment without a launcher's rank variables; PYTHONPATH is the repository root, then
    `extra_path`."""
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER_VARS}
    env["PYTHONPATH"] = os.pathsep.join([p for p in (ROOT, extra_path) if p])
    return env


def kill_group(p):
    """SIGKILL to the session of a child started with start_new_session=True; the child is reaped."""
    os.killpg(p.pid, signal.SIGKILL)
    p.communicate()


def run_command(cmd, cwd, timeout, env):
    """`cmd` as a child in a session of its own; returns its stdout.  After `timeout` seconds its process group
    gets SIGTERM (a launcher forwards it to its ranks), 30 s later SIGKILL, and the test fails; so it does when
    the child's exit code is not 0 (with the end of its stderr)."""
    p = subprocess.Popen(cmd, cwd=str(cwd), env=env, start_new_session=True, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGTERM)
        try:
            p.communicate(timeout=30)
        except subprocess.TimeoutExpired:
            kill_group(p)
        pytest.fail("timed out after %d s: %s" % (timeout, " ".join(cmd)))
    assert p.returncode == 0, (" ".join(cmd), err[-4000:])
    return out


def run_module(module, args, cwd, timeout, extra_path=None):
    """`python -m pulseportraiture_amd.<module> args` through run_command."""
    cmd = [sys.executable, "-m", "pulseportraiture_amd." + module] + list(args)
    return run_command(cmd, cwd, timeout, child_env(extra_path))


@pytest.fixture(scope="module")
def eng():
    """An engine of the importing module's own, closed after its tests."""
    from pulseportraiture_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def default_eng():
    """The process-wide engine the reference-shaped API runs on."""
    from pulseportraiture_amd.engine import default_engine
    return default_engine()


def dump_measured(env_name, measured):
    """`measured` as JSON to the path in the environment variable `env_name`; nothing when that is unset or
    `measured` is empty."""
    out = os.environ.get(env_name)
    if out and measured:
        with open(out, "w") as f:
            json.dump(measured, f, indent=1, sort_keys=True)


def measured_writer(env_name):
    """(MEASURED, fixture): a dict for a module's measured deviations, and the autouse module fixture that dumps
    it (dump_measured) after the module's tests.  Bind both at module level."""
    measured = {}

    @pytest.fixture(scope="module", autouse=True)
    def _write_measured():
        yield
        dump_measured(env_name, measured)
    return measured, _write_measured
