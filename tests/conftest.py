import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run by the driver with -m gpu)")
    config.addinivalue_line("markers", "experiments: a comparison kernel; runs against the ORL_BUILD_EXPERIMENTS library")


@pytest.fixture(autouse=True)
def _experiments_library(request):
    """Tests marked ``experiments`` run with the ORL_BUILD_EXPERIMENTS library loaded, every other test with the shipped one."""
    if request.node.get_closest_marker("experiments") is None:
        yield
        return
    from tests.helpers import experiments_library

    with experiments_library():
        yield


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")
