"""The stream and event logic of the sharded C entry points, exercised and shown to be NECESSARY (VERDICT r03 "next" 1a/1b).

The ranks are threads of one plain C++ process (tests/cabi/sharded_threads_demo.cpp: no Python, no torch) on this one GPU;
the library's ncclSend / ncclRecv calls are carried by tests/cabi/mock_rccl_async.cpp, a stand-in for librccl whose
ncclGroupEnd returns before anything has moved: every transfer is a device-to-device copy on a transfer stream of its own,
behind events of both sides' posting streams -- optionally behind a delay, so that the copy reads its source late.  What keeps
a send block intact until it has been read, and a received row unread until it has arrived, is then the library's own stream
ordering (qs_comm.hip: the waits on r_ready / x_ready / done), as on RCCL.

* positive: both entry points, every option, with a slow link (delay per transfer) and with a busy GPU (the caller's stream
  held back while the host posts the whole exchange): bit-identical to the single-GPU transform on every rank;
* negative: with ANY ONE of those waits left out (tuning key "comm_drop_wait", a test hook) the same runs come out WRONG.
  Without these the transport would prove nothing (the file-based stand-in of test_gpu_mock_rccl_ranks.py passes whatever
  the waits do).
"""

import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DELAY_US = 2000          # per transfer, on the transfer stream (a slow link)
STALL_US = 30000         # the caller's stream is held this long before the call (a busy GPU)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    libdir = os.path.join(ROOT, "quantum-systems_amd")
    assert os.path.exists(os.path.join(libdir, "libqs_amd.so")), "build the library first (__graft_entry__.build)"
    d = tmp_path_factory.mktemp("mock_rccl_async")
    mock = d / "librccl_async.so"
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-pthread",
                    os.path.join(ROOT, "tests", "cabi", "mock_rccl_async.cpp"), "-o", str(mock)], check=True, capture_output=True, timeout=300)
    exe = d / "sharded_threads_demo"
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi", "sharded_threads_demo.cpp"), "-L", libdir, "-l:libqs_amd.so",
                    f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, timeout=300)
    return str(mock), str(exe)


def run_demo(built, world, L, M, mode, chunk, coalesce, drop, stall_us, entry, delay_us):
    mock, exe = built
    # every stream of the process on a hardware queue of its own: with the runtime's default of four, streams share queues
    # and a delay kernel (or a stalled stream) holds back whatever was enqueued behind it on the same queue -- which would
    # serialise exactly the races this transport exists to expose.  32 queues hold the world^2 transfer streams plus two
    # streams per rank up to world = 4, the three-rank runs of the negative cases included; the five-rank positive case
    # shares queues, which can only serialise, never break, a correct ordering
    env = dict(os.environ, QS_AMD_RCCL_LIB=mock, QS_MOCK_RCCL_DELAY_US=str(delay_us), GPU_MAX_HW_QUEUES="32")
    cmd = [exe] + [str(x) for x in (world, L, M, mode, chunk, coalesce, drop, stall_us, entry)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    return res.returncode, res.stdout + res.stderr


# (world, L, M, mode, chunk_rows / nchunks, coalesce, entry)
POSITIVE = [
    (2, 12, 12, 0, 2, 0, 0), (2, 12, 12, 0, 2, 1, 0),
    (3, 14, 9, 1, 1, 0, 0), (3, 14, 9, 1, 1, 1, 0),
    (2, 10, 14, 1, 2, 1, 0),
    (3, 16, 16, 2, 0, 0, 0), (3, 16, 16, 2, 0, 1, 0),
    (4, 18, 18, 0, 1, 0, 0), (4, 18, 18, 0, 1, 1, 0),
    (5, 6, 6, 0, 1, 1, 0),                       # more ranks than some partitions have rows
    (2, 40, 40, 1, 0, 1, 0),
    (2, 12, 12, 0, 3, 0, 1), (3, 14, 9, 1, 4, 0, 1), (4, 18, 18, 0, 2, 0, 1),
]


@pytest.mark.parametrize("world,L,M,mode,chunk,coalesce,entry", POSITIVE)
@pytest.mark.parametrize("weather", ["slow_link", "busy_gpu"])
def test_every_rank_bit_identical_over_the_asynchronous_transport(built, world, L, M, mode, chunk, coalesce, entry, weather):
    delay, stall = (DELAY_US, 0) if weather == "slow_link" else (0, STALL_US)
    rc, text = run_demo(built, world, L, M, mode, chunk, coalesce, 0, stall, entry, delay)
    assert rc == 0 and text.count("RANK_OK") == world and "ALL_RANKS_OK" in text, text
    assert "mock rccl" not in text, text


# (drop bit, what it leaves out, entry, weather that exposes it, coalesce)
NEGATIVE = [
    (1, "rows: products of step t do not wait for the exchange of step t - 2 (send block overwritten)", 0, "slow_link", 0),
    (1, "the same, coalesced exchange", 0, "slow_link", 1),
    (2, "rows: the exchange of a step does not wait for the step's products (send block read early)", 0, "busy_gpu", 0),
    (2, "the same, coalesced exchange", 0, "busy_gpu", 1),
    (4, "rows: the closing products do not wait for the exchange (rows read before they arrived)", 0, "slow_link", 0),
    (4, "the same, coalesced exchange", 0, "slow_link", 1),
    (8, "slab entry: the closing product of a chunk does not wait for the chunk's rows", 1, "slow_link", 0),
    (16, "slab entry: the exchange of a chunk does not wait for the chunk's products", 1, "busy_gpu", 0),
]


@pytest.mark.parametrize("drop,what,entry,weather,coalesce", NEGATIVE)
def test_a_missing_stream_wait_is_caught(built, drop, what, entry, weather, coalesce):
    delay, stall = (DELAY_US, 0) if weather == "slow_link" else (0, STALL_US)
    world, L, M, mode, chunk = (3, 12, 12, 0, 1) if entry == 0 else (3, 12, 12, 0, 3)      # rows: four steps per rank
    # the control: the same run with every wait in place is right ...
    rc, text = run_demo(built, world, L, M, mode, chunk, coalesce, 0, stall, entry, delay)
    assert rc == 0 and "ALL_RANKS_OK" in text, text
    # ... and wrong without this one.  (A race is exposed by timing: the delay / the stall make it all but certain, every run so far
    # showed it at the first attempt; up to three attempts keep a slow box from turning the control into a flaky test.)
    for attempt in range(3):
        rc, text = run_demo(built, world, L, M, mode, chunk, coalesce, drop, stall * (attempt + 1), entry, delay * (attempt + 1))
        if rc == 1:
            break
    assert rc == 1 and "SOME_RANK_WRONG" in text and "RANK_WRONG" in text, f"{what}: NOT caught\n{text}"
