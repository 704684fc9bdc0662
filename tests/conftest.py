import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
os.environ.setdefault("GSX_LOG_LEVEL", "warning")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture
def sock_dir():
    """A short directory for unix sockets: sun_path holds 107 characters, and pytest's ``tmp_path`` (temp dir + user +
    run + test name) can use most of them before the socket's own name is added."""
    import shutil
    import tempfile

    base = tempfile.gettempdir()
    d = Path(tempfile.mkdtemp(prefix="gsx", dir=base if len(base) <= 48 else "/tmp"))
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session", autouse=True)
def _native_built():
    """Build the native extensions in-tree once per session (no-op when up to date)."""
    from gpushare_scheduler_extender_amd.utils.build import build_native

    build_native(["engine", "mxdev"])
    yield
