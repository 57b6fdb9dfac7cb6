"""Coordinator bookkeeping when a rank is replaced during a re-rendezvous (sched/cluster.py), without
processes: a worker whose teardown hangs leaves by itself while the coordinator is about to force-replace it.
Whichever of the two notices first, the rank gets exactly one replacement, that replacement is never killed,
and a connected replacement that dies before it joined the group is replaced in turn."""
import threading
import types

import pytest

from comfy_gen_server_amd.sched import cluster


class _Conn:
    def __init__(self):
        self.sent = []

    def send_bytes(self, b):
        self.sent.append(b)


class _Proc:
    def __init__(self, exited=True):
        self.exited, self.killed = exited, False

    def wait(self, timeout=None):
        if not self.exited:
            raise cluster.subprocess.TimeoutExpired("worker", timeout)
        return 0

    def poll(self):
        return 0 if self.exited else None

    def kill(self):
        self.killed = True


@pytest.fixture
def coord(monkeypatch):
    # Keep in sync with Coordinator.__init__: this sets by hand every attribute that _rank_died and
    # _force_replace read (no sockets, threads or executors), and stubs _spawn_replacement. An AttributeError
    # here means one of them reads a new attribute -- add it below.
    c = object.__new__(cluster.Coordinator)
    c.world, c.respawn = 4, True
    c.cv = threading.Condition()
    c.dead, c.conns, c.locks, c.busy = set(), {}, {}, {}
    c._inflight, c._retries, c.spmd_waiting, c._respawns, c._spawned, c.procs = {}, {}, {}, {}, {}, []
    c.comm = types.SimpleNamespace(store=lambda: None)
    c.spawned = []        # (rank, replacement process)

    def spawn(r):         # what _spawn_replacement records, without starting a process
        p = _Proc(exited=False)
        c._spawned[r] = p
        cluster._LAUNCH.setdefault("procs", {})[r] = p
        c._respawns[r] = c._respawns.get(r, 0) + 1
        c.spawned.append((r, p))
    c._spawn_replacement = spawn
    monkeypatch.setattr(cluster, "_LAUNCH", {"argv": [], "pypath": "", "procs": {}})
    return c


def _member(c, r, exited=True):
    conn, proc = _Conn(), _Proc(exited)
    c.conns[r], c.locks[r] = conn, threading.Lock()
    cluster._LAUNCH["procs"][r] = proc
    return conn, proc


def _replacement_connects(c, r):
    conn = _Conn()
    c.conns[r], c.locks[r] = conn, threading.Lock()
    return conn


def test_reader_notices_first_then_force_replace_spares_the_replacement(coord):
    c = coord
    old_conn, old_proc = _member(c, 2)                 # exits by itself (hung teardown)
    c._rank_died(2, old_conn)                          # its connection dropped: reader thread
    assert c.dead == {2} and [r for r, _ in c.spawned] == [2]
    new_conn = _replacement_connects(c, 2)
    c._force_replace(2, old_conn, old_proc)            # the re-rendezvous thread, late
    new_proc = c.spawned[0][1]
    assert not new_proc.killed and new_conn.sent == [] and old_conn.sent == []
    assert [r for r, _ in c.spawned] == [2] and c.conns[2] is new_conn and c.dead == {2}


def test_force_replace_first_then_the_readers_report_is_stale(coord):
    c = coord
    old_conn, old_proc = _member(c, 2, exited=False)   # does not leave by itself: asked to exit, then killed
    c._force_replace(2, old_conn, old_proc)
    assert old_proc.killed and len(old_conn.sent) == 1 and b"exit" in old_conn.sent[0]
    assert c.dead == {2} and [r for r, _ in c.spawned] == [2] and 2 not in c.conns
    c._rank_died(2, old_conn)                          # the reader's EOF for the same death
    c._rank_died(2)                                    # a failed send to the same rank
    assert [r for r, _ in c.spawned] == [2]


def test_connected_replacement_that_dies_is_replaced_again(coord):
    c = coord
    old_conn, _ = _member(c, 1)
    c._rank_died(1, old_conn)
    new_conn = _replacement_connects(c, 1)
    c._rank_died(1, old_conn)                          # stale: ignored
    assert [r for r, _ in c.spawned] == [1]
    c._rank_died(1, new_conn)                          # the replacement itself dropped before it joined
    assert [r for r, _ in c.spawned] == [1, 1] and c.dead == {1} and 1 not in c.conns
