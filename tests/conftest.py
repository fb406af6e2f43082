import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


@pytest.fixture
def tmp_path():
    """A short per-test directory instead of pytest's own.  The tests bind the
    pod servers' Unix sockets under it, and a socket path holds at most 107
    bytes: pytest's <TMPDIR>/pytest-of-<user>/pytest-N/<test name>/ exceeds
    that wherever the temporary directory itself has a long path."""
    import shutil
    import tempfile

    base = "/tmp" if os.access("/tmp", os.W_OK | os.X_OK) else None
    d = Path(tempfile.mkdtemp(prefix="nos_t_", dir=base))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU")
    config.addinivalue_line("markers", "slow: long-running simulation test")


def pytest_collection_modifyitems(config, items):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)
