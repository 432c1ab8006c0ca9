import os
import sys

# The in-process tensor-parallel test group runs up to 8 ranks as host threads of ONE process; every rank's gather kernel
# polls for its peers on the device, so each rank's stream needs its own hardware queue (the HIP runtime's default is 4 queues
# per process, onto which streams are multiplexed: a polling kernel would then block the peer queued behind it).  Must be set
# before the HIP runtime initialises.  Production runs one process per GPU and does not need this.  A value inherited from the
# environment is overridden, not kept: with 4 queues (a common setting) the 8-rank groups' gathers time out.  The tests' child
# processes (scripts/debug_tp_fold.py) inherit it.
os.environ["GPU_MAX_HW_QUEUES"] = "32"

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402


def pytest_collection_modifyitems(config, items):
    """The in-process tensor-parallel groups (up to 8 ranks = 8 polling gather kernels that must be co-resident, one hardware
    queue each) run FIRST: late in a long-lived process the HIP runtime has handed hardware queues to graph executors and
    destroyed streams, two rank streams can end up on one queue, and a rank then waits for a peer queued behind itself until the
    gather's bounded spin gives up (seen once in round 3 as test 105 of 172; the same tests pass alone).  One process per GPU —
    the production layout — has one stream per process and no such coupling."""
    def tp_first(item):
        return 0 if ("test_gpu_tp.py" in item.nodeid or "tp8" in item.nodeid) else 1
    items.sort(key=tp_first)          # stable: everything else keeps its order


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="session")
def orc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c
