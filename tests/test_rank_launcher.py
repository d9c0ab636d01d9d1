"""apps/rank_launcher.hpp (the fork / pipe / wait logic of ecc_sharded_step) cannot hang when a
rank fails: CPU tests with a stand-alone probe (tests/rank_launcher_probe.cpp: its own main, only
the launcher header, no libecc) whose four ranks never touch a GPU.

A rank that dies before the id exchange must give the readers EOF, and one that fails later must
get its siblings (which may sit in a collective that can no longer complete) terminated: both
cases end far sooner than the 60 s the surviving ranks would sleep, and leave no process behind.
"""
import os
import signal
import subprocess
import time
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
APPS = ROOT / "event-camera-clustering-and-optical-flow-estimation_amd" / "apps"
N_RANKS, BLOB = 4, bytes((i * 7 + 3) & 255 for i in range(128))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launcher") / "rank_launcher_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{APPS}", "-o", str(exe),
                    str(Path(__file__).with_name("rank_launcher_probe.cpp"))], check=True, timeout=120)
    return exe


def _run(probe, mode, tmp_path):
    """(exit status, seconds, stdout).  The probe leads a process group of its own, so that the
    group is empty afterwards exactly when no rank outlives the launcher."""
    out = tmp_path / "stdout.txt"
    t0 = time.monotonic()
    with open(out, "wb") as f:
        p = subprocess.Popen([str(probe), mode], stdout=f, start_new_session=True)
    try:
        try:
            rc = p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{mode}: the launcher still runs after 30 s")
        seconds = time.monotonic() - t0
        with pytest.raises(ProcessLookupError):  # no rank left reading or sleeping
            os.killpg(p.pid, 0)
        return rc, seconds, out.read_text()
    finally:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.wait()


def test_rank0_dying_before_the_id_exchange_ends_every_rank(probe, tmp_path):
    rc, seconds, _ = _run(probe, "rank0_dies_early", tmp_path)
    assert rc != 0
    assert seconds < 20, seconds


def test_rank_failing_after_the_id_exchange_ends_its_siblings(probe, tmp_path):
    rc, seconds, _ = _run(probe, "rank2_fails_late", tmp_path)
    assert rc != 0
    assert seconds < 20, seconds


def test_all_ranks_succeed_and_receive_the_same_id(probe, tmp_path):
    rc, _, out = _run(probe, "all_ok", tmp_path)
    assert rc == 0
    assert sorted(out.splitlines()) == [f"rank {r} {BLOB.hex()}" for r in range(N_RANKS)]
