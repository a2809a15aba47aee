"""The composed reference of the two device-resident chains (tests/path_ref.py)
pinned on the CPU, before any kernel is compared with it:

  - the loopback property: what goes into the send chain as a Tun.Read
    super-packet comes out of the receive chain's GRO as one buffer with the
    same L4 payload and the same virtio header;
  - the scenario's proof that no joint is vacuous (path_ref.check_scenario),
    at the seeds and strides that tests/test_gpu_path.py uses;
  - the tun parts of the chain (the GSO split and GRO) through the second
    restatement, oracle/py_restatement.py, byte for byte.  GRO's input here is
    a kind no corpus has: slots with a transport header in front of the packet
    and stale padding and a tag behind it."""
import numpy as np
import pytest

import path_ref
import py_restatement as py

PARAMS = [(4096, 4096), (4112, 4099)]  # (stride, in_stride) of tests/test_gpu_path.py
SEED = 20261019


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-{p[1]}")
def ref(request):
    stride, in_stride = request.param
    return path_ref.run_reference(SEED, stride, in_stride)  # check_scenario runs inside


def test_scenario_is_not_vacuous(ref):
    s, snd, rcv = ref.s, ref.snd, ref.rcv
    path_ref.check_scenario(s, snd, ref.plan, rcv)
    # the figures the chain tests' documentation quotes
    by_job = {}
    for j, m, first, length, gso in snd.wire:
        by_job.setdefault(j, []).append((length, gso))
    assert by_job[0] == [(3680, 272)] and by_job[2] == [(3680, 272)]
    assert by_job[1] == [(4096, 304)]
    assert by_job[3] == [(3216, 1072), (1040, -1)]
    assert by_job[4] == [(336, -1)]
    assert by_job[8] == [(3176, 1532)]
    assert ref.plan.n_batches == 6 and len(ref.n_in) == 6 * 128


def test_loopback_property(ref):
    """Jobs 2, 3, 4, 9 and 10: neither dropped nor tampered with."""
    s, rcv = ref.s, ref.rcv
    assert path_ref.check_loopback(s, rcv, rcv.arena) == 5
    # and the property can fail: one payload byte off in the final arena
    bad = rcv.arena.copy()
    first, n_write = int(rcv.gro_calls["first"][0]), int(rcv.n_write[0])
    h = rcv.gro_bufs[first + int(rcv.to_write[first + n_write - 1])]  # the call's last buffer: job 2's
    bad[int(h["off"]) + int(h["len"]) - 1] ^= 1
    with pytest.raises(AssertionError):
        path_ref.check_loopback(s, rcv, bad)
    # the jobs that were tampered with or dropped do not come back whole
    total = sum(len(b) for b in path_ref.written(s, rcv, rcv.arena))
    whole = sum(16 + s.jobs[j].total for j in s.loopback_jobs)
    assert total == whole + (16 + 240) + (16 + 2700 - 2 * 200)  # job 1: its first segment, and the rest after the gap


def test_wire_is_the_same_function_of_equal_inputs(ref):
    land, n_in, gso = path_ref.wire(ref.s, ref.plan, ref.snd.arena.copy(), ref.snd.msg_len.copy(), ref.snd.msg_gso.copy())
    assert np.array_equal(land, ref.land) and np.array_equal(n_in, ref.n_in) and np.array_equal(gso, ref.gso)
    assert (n_in != 0).sum() == len(ref.plan.order) and (gso != 0).sum() == sum(w[4] > 0 for w in ref.snd.wire)


def _same(a, b, names):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert np.array_equal(x, y), name


def test_tun_parts_through_the_python_restatement(ref):
    s = ref.s
    snd = path_ref.send_ref(s, handle_virtio_read=py.run_handle_virtio_read)
    _same(snd, ref.snd, ("arena_split", "sizes", "count", "status", "peer", "out_len", "arena", "n_msgs", "msg_first",
                         "msg_len", "msg_gso"))
    rcv = path_ref.recv_ref(s, ref.land, ref.n_in, ref.gso, handle_gro=py.run_handle_gro)
    _same(rcv, ref.rcv, ("arena_opened", "verdict", "gro_status", "n_write", "to_write", "gro_bufs", "arena"))
    assert (ref.rcv.arena != ref.rcv.arena_opened).any()  # GRO wrote: the comparison above saw its bytes
