"""The direct xGMI halo kernels (csrc/ibh_halo.hip, csrc/ibh_halo_dev.h, the exchange part of ``k_step_quad``) in ONE
process on one stream, against the numpy model of tests/halo_loopback.py (pinned by tests/test_halo_loopback_model.py):
several peers per rank, empty segments, the 16-peer bound, the second trip of the grid-stride loops past the 64- and
256-workgroup caps, ``ld > n``, nv 1..7, an odd number of exchanges per captured graph, the time-out bit, and the four
entry points nothing else calls (``ibh_halo_push``, ``ibh_halo_pull``, ``ibh_flag_signal``, ``ibh_flag_wait``).

Every comparison is ``np.array_equal`` on ``uint32`` views of whole storages (field with padding, receive buffers).
Every wait gets ``max_spins <= 256``; outside the two time-out tests the flags are set before the wait starts (the signal
is earlier on the stream or in the same kernel), and ``state[2] == 0`` is asserted at the end: a protocol error shows as
a status bit after microseconds, never as a long spin.  What one process cannot show -- visibility across processes and
devices, ranks running concurrently -- stays with tests/test_gpu_halo_xgmi.py and the multi-GPU runs."""
import numpy as np
import pytest
import torch

import halo_loopback as hl
import ibamd
from conftest import advection_mesh, rae_mesh
from ibamd import _lib

pytestmark = pytest.mark.gpu

S = hl.MAX_SPINS


@pytest.fixture
def dev():
    d = hl.Device()
    yield d
    d.close()


def _words(rng, shape):
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)


def _state(dev, state):
    return dev.words(state)[:5].tolist()


# ---- a. ibh_halo_exchange, one rank as its own peers ---------------------------------------------------------------
@pytest.mark.parametrize("case", hl.EXCHANGE_CASES, ids=lambda c: c[0])
def test_exchange_self_loop(dev, case):
    _, seg, perm, nv, pad = case
    loop = hl.exchange_loop(seg, perm, nv, pad).check()
    L = hl.LoopDevice(dev, loop)
    rng = np.random.default_rng(100 + nv + pad)
    f = _words(rng, (nv, loop.ld))
    f0 = f.copy()
    F, state = dev.tensor(f), dev.state()
    L.fill_bufs(hl.SENTINEL)
    bufs = np.full((2, loop.buf_words), hl.SENTINEL, dtype=np.uint32)
    for k in range(5):
        f[:, loop.send_all] = _words(rng, (nv, loop.total))      # new values to send before every launch
        dev.upload(F, f)
        want = loop.expected(f)
        loop.model(f, bufs, k & 1)
        L.exchange(F, state)
        got, gb = dev.words(F), L.read_bufs()
        assert np.array_equal(got, want), f"launch {k}: field"
        assert np.array_equal(got, f), f"launch {k}: field against the model through the buffers"
        assert np.array_equal(gb, bufs), f"launch {k}: receive buffers"
        if k == 0:
            assert np.all(gb[1] == hl.SENTINEL), "the parity not in use was written"
    assert _state(dev, state) == [5, 5, 0, 0, 0]
    assert np.all(L.read_flags()[:loop.K] == 5)
    if loop.total == 0:
        assert np.array_equal(dev.words(F), f0)


# ---- b. argument checks, before any launch -------------------------------------------------------------------------
def test_argument_checks_launch_nothing(dev):
    loop = hl.exchange_loop(**hl.ARGCHECK_LOOP).check()
    L = hl.LoopDevice(dev, loop)
    v, nv, ld, K = dev.vp, loop.nv, loop.ld, loop.K
    rng = np.random.default_rng(1)
    f = _words(rng, (nv, ld))
    F, state = dev.tensor(f), dev.state()
    dev.upload(state, np.array([6, 6, 0, 0, 0, 0, 0, 0], dtype=np.int32))
    L.fill_bufs(hl.SENTINEL)
    seg17 = dev.segs([0] * 18)
    p17 = dev.ptrs([L.recv] * 17)
    fl17 = dev.ptrs([L.flags] * 17)
    down = dev.segs([0, 9, 5, 19])
    st = v(state)

    def push(nv=nv, send_all=L.send_all, n=K, seg=L.sseg, dst=L.dst[0], flags=L.sflags):
        return dev.call("ibh_halo_push", v(F), nv, ld, v(send_all), n, v(seg), v(dst), v(flags), st)

    def pull(nv=nv, recv_all=L.recv_all, n=K, seg=L.rseg, flags=L.rflags):
        return dev.call("ibh_halo_pull", v(F), nv, ld, v(recv_all), v(L.src[0]), n, v(seg), v(flags), st, S)

    def xchg(nv=nv, send_all=L.send_all, ns=K, sseg=L.sseg, dst=L.dst, sfl=L.sflags, nr=K, rseg=L.rseg, rfl=L.rflags):
        return dev.call("ibh_halo_exchange", v(F), nv, ld, v(send_all), ns, v(sseg), v(dst[0]), v(dst[1]), v(sfl),
                        v(L.recv_all), v(L.src[0]), v(L.src[1]), nr, v(rseg), v(rfl), st, S)

    bad = [
        lambda: push(n=17, seg=seg17, dst=p17, flags=fl17),
        lambda: pull(n=17, seg=seg17, flags=fl17),
        lambda: xchg(ns=17, sseg=seg17, dst=[p17, p17], sfl=fl17),
        lambda: xchg(nr=17, rseg=seg17, rfl=fl17),
        lambda: push(seg=down), lambda: pull(seg=down), lambda: xchg(sseg=down), lambda: xchg(rseg=down),
        lambda: push(nv=0), lambda: pull(nv=0), lambda: xchg(nv=0),
        lambda: xchg(send_all=None), lambda: push(send_all=None), lambda: pull(recv_all=None),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.IbhError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # no peers: nothing to do, nothing launched
    assert push(n=0) == 0 and pull(n=0) == 0 and xchg(ns=0, nr=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.words(F), f)
    assert np.all(L.read_bufs() == hl.SENTINEL) and np.all(L.read_flags() == 0)
    assert dev.words(state).tolist() == [6, 6, 0, 0, 0, 0, 0, 0]


# ---- c. ibh_halo_push / ibh_halo_pull, W ranks in one process ------------------------------------------------------
@pytest.fixture(scope="module")
def cuts():
    out = {}
    for name, msh, world in (("adv4", advection_mesh(2e-2), 4), ("rae8", rae_mesh(), 8)):
        dom, plans = hl.real_plans(msh, world)
        out[name] = (len(msh), dom, plans)
    return out


def _lds(plans, pad):
    return {r: plans[r].nc + pad for r in plans}


def _check_states(dev, R, n):
    for r in R.plans:
        assert _state(dev, R.state[r]) == [n, n, 0, 0, 0], f"rank {r}"


@pytest.mark.parametrize("order", ["ranks_up", "ranks_down"])
@pytest.mark.parametrize("nv,pad", [(1, 0), (1, 5), (5, 0), (5, 5)])
@pytest.mark.parametrize("cut", ["adv4", "rae8"])
def test_push_pull_real_plans(dev, cuts, cut, nv, pad, order):
    ncells, dom, plans = cuts[cut]
    lds = _lds(plans, pad)
    R = hl.RankSet(dev, plans, nv, lds)
    ranks = sorted(plans, reverse=order == "ranks_down")
    rng = np.random.default_rng(200 + nv + pad)
    F = {r: dev.tensor(np.zeros((nv, lds[r]), dtype=np.uint32)) for r in plans}
    mbufs = None
    for rnd in range(5):
        G = _words(rng, (nv, ncells))                      # the owners' values change every round
        fields = {r: hl.rank_storage(G, dom.partitions[r], nv, lds[r]) for r in plans}   # skirts poisoned
        for r in plans:
            dev.upload(F[r], fields[r])
        mbufs = hl.model_exchange(plans, fields, nv, rnd & 1, mbufs)
        for r in ranks:
            R.push(r, F[r], rnd & 1)
        for r in ranks:
            R.pull(r, F[r], rnd & 1, S)
        for r in plans:
            got = dev.words(F[r])
            assert np.array_equal(got, hl.expected_storage(G, dom.partitions[r], nv, lds[r])), (rnd, r)
            assert np.array_equal(got, fields[r]), (rnd, r)
            assert np.array_equal(R.read_bufs(r), mbufs[r]), (rnd, r)
    _check_states(dev, R, 5)


@pytest.mark.parametrize("cut,nv,pad", [("adv4", 1, 0), ("rae8", 5, 5)])
def test_push_one_step_ahead(dev, cuts, cut, nv, pad):
    """The double-buffer argument of the ``XgmiHalo`` docstring: a rank may push round k+1 before its peers have pulled
    round k.  Rounds k and k+1 are pushed by every rank before any pull; each pull delivers its own round's values."""
    ncells, dom, plans = cuts[cut]
    lds = _lds(plans, pad)
    R = hl.RankSet(dev, plans, nv, lds)
    rng = np.random.default_rng(300 + nv)
    F = {r: dev.tensor(np.zeros((nv, lds[r]), dtype=np.uint32)) for r in plans}
    mbufs = None
    for k in (0, 2):                                        # the second pair reuses both parities
        Gs = [_words(rng, (nv, ncells)), _words(rng, (nv, ncells))]
        for j in (0, 1):
            fields = {r: hl.rank_storage(Gs[j], dom.partitions[r], nv, lds[r]) for r in plans}
            for r in plans:
                dev.upload(F[r], fields[r])
            mbufs = hl.model_exchange(plans, fields, nv, (k + j) & 1, mbufs, pull=False)
            for r in sorted(plans):
                R.push(r, F[r], (k + j) & 1)
        for j in (0, 1):
            hl.model_exchange(plans, fields, nv, (k + j) & 1, mbufs, push=False)
            for r in sorted(plans):
                R.pull(r, F[r], (k + j) & 1, S)
            for r in plans:
                part = dom.partitions[r]
                want = hl.expected_storage(Gs[j], part, nv, lds[r])      # skirt rows: round k+j ...
                want[:, part.image_in_domain] = Gs[1][:nv, np.asarray(part.domain)[part.image_in_domain]]  # owned: k+1
                got = dev.words(F[r])
                assert np.array_equal(got, want), (k, j, r)
                assert np.array_equal(got, fields[r]), (k, j, r)
        for r in plans:
            assert np.array_equal(R.read_bufs(r), mbufs[r]), (k, r)
    _check_states(dev, R, 4)


@pytest.mark.parametrize("nv", [1, 3])
def test_push_pull_past_the_workgroup_caps(dev, nv):
    """65 536 + 3 rows from rank 1 to rank 2: the second trip of push (256 workgroups) and trips 2..5 of pull (64)."""
    plans = hl.synthetic_two_rank_plans(65536 + 3, 5, seed=5)
    lds = {1: plans[1].nc, 2: plans[2].nc + 5}
    R = hl.RankSet(dev, plans, nv, lds)
    rng = np.random.default_rng(400 + nv)
    F = {r: dev.tensor(np.zeros((nv, lds[r]), dtype=np.uint32)) for r in plans}
    mbufs = None
    for rnd in range(3):
        fields = {r: _words(rng, (nv, lds[r])) for r in plans}
        for r in plans:
            dev.upload(F[r], fields[r])
        sent = fields[1][:, plans[1].send[2]].copy()
        mbufs = hl.model_exchange(plans, fields, nv, rnd & 1, mbufs)
        for r in (1, 2):
            R.push(r, F[r], rnd & 1)
        for r in (1, 2):
            R.pull(r, F[r], rnd & 1, S)
        for r in plans:
            assert np.array_equal(dev.words(F[r]), fields[r]), (rnd, r)
            assert np.array_equal(R.read_bufs(r), mbufs[r]), (rnd, r)
        assert np.array_equal(fields[2][:, plans[2].recv[1]], sent)
    _check_states(dev, R, 3)


# ---- d. ibh_flag_signal / ibh_flag_wait ----------------------------------------------------------------------------
def _flag_tables(dev, n):
    flags = dev.alloc(64)
    order = np.random.default_rng(n).permutation(64)[:max(n, 1)]          # scattered slots
    slots = torch.tensor([flags + 4 * int(s) for s in order], dtype=torch.int64, device=dev.dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev.dev)          # [0] signal, [1] wait
    status = torch.zeros(1, dtype=torch.int32, device=dev.dev)
    return flags, order, slots, counters, status


@pytest.mark.parametrize("n", [0, 1, 3, 64])
def test_flag_signal_then_wait(dev, n):
    flags, order, slots, counters, status = _flag_tables(dev, n)
    v = dev.vp
    for k in (1, 2, 3):
        dev.call("ibh_flag_signal", v(counters.data_ptr()), v(slots), n)
        dev.call("ibh_flag_wait", v(counters.data_ptr() + 4), v(slots), n, S, v(status))
        got = dev.read(flags, 64)
        want = np.zeros(64, dtype=np.uint32)
        want[order[:n]] = k
        assert np.array_equal(got, want)
        assert dev.words(counters).tolist() == [k, k]
        assert dev.words(status).tolist() == [0]


def test_flag_entry_points_refuse_65_slots(dev):
    flags, order, slots, counters, status = _flag_tables(dev, 64)
    v = dev.vp
    with pytest.raises(_lib.IbhError):
        dev.call("ibh_flag_signal", v(counters.data_ptr()), v(slots), 65)
    with pytest.raises(_lib.IbhError):
        dev.call("ibh_flag_wait", v(counters.data_ptr() + 4), v(slots), 65, S, v(status))
    torch.cuda.synchronize()
    assert np.all(dev.read(flags, 64) == 0)
    assert dev.words(counters).tolist() == [0, 0] and dev.words(status).tolist() == [0]


# ---- e. the time-out report: a bounded wait of 64 polls, run once --------------------------------------------------
def test_flag_wait_reports_a_time_out(dev):
    flags, order, slots, counters, status = _flag_tables(dev, 3)
    v = dev.vp
    dev.call("ibh_flag_wait", v(counters.data_ptr() + 4), v(slots), 3, 64, v(status))     # nobody signalled
    assert dev.words(status)[0] & 1 == 1
    assert dev.words(counters).tolist() == [0, 1]


def test_pull_reports_a_time_out_and_goes_on(dev):
    """A pull without a push gives up after ``max_spins`` polls: status bit 0, the wait sequence advanced, and the
    buffer's contents (the sentinel) unpacked -- the kernel goes on, as include/ibhip.h says.

    Afterwards: the sequence numbers are monotonic, so the pull of round 2 waits for the SECOND signal of its peers.  The
    push that round 1 never saw therefore arrives late (its flags then equal the wait sequence, as they would for a late
    peer); then the status is cleared (``reset_health``), and after ONE more push the next pull passes with status 0."""
    loop = hl.exchange_loop(**hl.TIMEOUT_LOOP).check()
    L = hl.LoopDevice(dev, loop)
    rng = np.random.default_rng(9)
    f = _words(rng, (loop.nv, loop.ld))
    F, state = dev.tensor(f), dev.state()
    L.fill_bufs(hl.SENTINEL)
    bufs = np.full((2, loop.buf_words), hl.SENTINEL, dtype=np.uint32)
    L.pull(F, state, 0, 64)                                  # round 1: nobody pushed
    assert _state(dev, state) == [0, 1, 1, 0, 0]
    loop.model(f, bufs, 0, push=False)
    assert np.all(f[:, loop.recv_all] == hl.SENTINEL)
    assert np.array_equal(dev.words(F), f)
    L.push(F, state, 0)                                      # the late push of round 1
    loop.model(f, bufs, 0, pull=False)
    state[2] = 0                                             # XgmiHalo.reset_health
    f[:, loop.send_all] = _words(rng, (loop.nv, loop.total))
    dev.upload(F, f)
    want = loop.expected(f)
    L.push(F, state, 1)                                      # round 2
    L.pull(F, state, 1, S)
    loop.model(f, bufs, 1)
    assert _state(dev, state) == [2, 2, 0, 0, 0]
    assert np.array_equal(dev.words(F), want) and np.array_equal(want, f)
    assert np.array_equal(L.read_bufs(), bufs)


# ---- f. graph replay with an odd number of exchanges ---------------------------------------------------------------
def test_graph_of_three_exchanges_mixed_with_eager(dev):
    """The buffer parity follows the device-side sequence number: a graph of THREE exchanges starts on the other parity
    at every second replay, and eager launches in between shift it again.  (A parity baked into the launches at capture
    would repeat the parities of the capture.)"""
    loop = hl.exchange_loop(**hl.GRAPH_LOOP).check()
    nv = loop.nv
    rng = np.random.default_rng(21)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L = hl.LoopDevice(dev, loop)
        fh = rng.uniform(-1, 1, size=(nv, loop.ld)).astype(np.float32)     # finite: torch adds to them in the graph
        F, state = dev.tensor(fh), dev.state()
        sidx = dev.tensor(loop.send_all).long()
        L.fill_bufs(hl.SENTINEL)
        bufs = np.full((2, loop.buf_words), hl.SENTINEL, dtype=np.uint32)
        seq = [0]

        def bump():                                           # in place, on the stream: the send rows change
            F.index_copy_(1, sidx, F.index_select(1, sidx) + 1.0)

        def model_launch():
            loop.model(fh.view(np.uint32), bufs, seq[0] & 1)
            seq[0] += 1

        def compare(what):
            assert np.array_equal(dev.words(F), fh.view(np.uint32)), what
            assert np.array_equal(L.read_bufs(), bufs), what
            assert _state(dev, state) == [seq[0], seq[0], 0, 0, 0], what

        def eager(what):
            fh[:, loop.send_all] = rng.uniform(-1, 1, size=(nv, loop.total)).astype(np.float32)
            dev.upload(F, fh)
            bump()
            fh[:, loop.send_all] += np.float32(1.0)
            L.exchange(F, state)
            model_launch()
            compare(what)

        def replay(what):
            assert seq[0] & 1 == want_parity.pop(0), what
            fh[:, loop.send_all] = rng.uniform(-1, 1, size=(nv, loop.total)).astype(np.float32)
            dev.upload(F, fh)
            graph.replay()
            for j in range(3):
                if j:
                    fh[:, loop.send_all] += np.float32(1.0)
                model_launch()
            compare(what)

        eager("eager 1")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for j in range(3):
                if j:
                    bump()
                L.exchange(F, state)
        want_parity = [1, 1, 0]
        replay("replay 1")
        eager("eager 2")
        replay("replay 2")
        replay("replay 3")
        assert seq[0] == 11 and _state(dev, state)[:2] == [11, 11]
        del graph
    torch.cuda.current_stream().wait_stream(side)


# ---- g. the fused step, ibh_step_advection_xgmi --------------------------------------------------------------------
@pytest.fixture(scope="module")
def rae_rank1():
    """Partition 1 of 2 of the 37 k-cell RAE2822 mesh (what scripts/rehearse_xgmi.py runs the fused step on)."""
    msh = rae_mesh()
    dom = ibamd.Domain(msh, max_partition_size=hl.partition_size(len(msh), 2), boundaries=False, only=[1])
    part = dom.partitions[1]
    return part, ibamd.to_backend(part, ibamd.hip)


@pytest.mark.parametrize("K", [1, 3, 16])
def test_fused_step_self_loop(dev, rae_rank1, K):
    from ibamd import backend as B
    part, dpart = rae_rank1
    assert dpart.info["image_blocks_all_eligible"] and dpart.info["image_quads"] > 0
    loop = hl.fused_loop(part, K).check()
    L = hl.LoopDevice(dev, loop)
    nc = dpart.nc
    xc = part.centers.astype(np.float64)
    base = (np.sin(2 * np.pi * xc[:, 0]) * np.cos(2 * np.pi * xc[:, 1])
            + 0.1 * np.sin(37.0 * xc[:, 0] + 11.0 * xc[:, 1])).astype(np.float32)
    Ch = np.stack([np.ones(nc, np.float32), (0.5 + 0.2 * np.cos(5.0 * xc[:, 0])).astype(np.float32)], axis=1)
    C = ibamd.hip(Ch)
    Cf, _, ldc = B._field(C, nc)
    img = np.asarray(part.image_in_domain)
    rng = np.random.default_rng(31 + K)
    u = ibamd.hip(base)
    ud = torch.empty(nc, dtype=torch.float32, device=dev.dev)
    ref = torch.empty(nc, dtype=torch.float32, device=dev.dev)
    state = dev.state()
    fstate = torch.zeros(2, dtype=torch.int64, device=dev.dev)
    L.fill_bufs(hl.SENTINEL)
    bufs = np.full((2, loop.buf_words), hl.SENTINEL, dtype=np.uint32)
    v = dev.vp
    for step in range(3):
        uh = base.copy()
        uh[loop.recv_all] = np.nan                                        # stale skirt rows
        uh[loop.send_all] = rng.uniform(-1, 1, loop.total).astype(np.float32)
        dev.upload(u, uh)
        # expected, built outside the kernel: the rows move, then the image-only sweep of the library reads them
        u_ref = loop.expected(uh.view(np.uint32).reshape(1, nc)).reshape(nc).view(np.float32)
        assert np.all(np.isfinite(u_ref))
        ref.fill_(float("nan"))
        ibamd.residual_advection(dpart, ibamd.hip(u_ref), C, out=ref, flags=ibamd.IBH_IMAGE_ONLY)
        loop.model(uh.view(np.uint32).reshape(1, nc), bufs, step & 1)
        ud.fill_(float("nan"))
        dev.call("ibh_step_advection_xgmi", dpart.handle, v(u), v(Cf), ldc, v(ud), *L.exchange_args(state, S), v(fstate))
        got_u = dev.words(u)
        assert np.array_equal(got_u, u_ref.view(np.uint32)), f"step {step}: u"
        assert np.array_equal(got_u, uh.view(np.uint32)), f"step {step}: u against the model through the buffers"
        assert np.array_equal(dev.words(ud)[img], dev.words(ref)[img]), f"step {step}: ud on the image rows"
        assert np.all(np.isfinite(dev.words(ud).view(np.float32)[img]))
        assert np.array_equal(L.read_bufs(), bufs), f"step {step}: receive buffers"
        assert _state(dev, state) == [step + 1, step + 1, 0, 0, 0]


def test_fused_step_argument_checks_launch_nothing(dev, rae_rank1):
    """The fused step takes the same tables as ``ibh_halo_exchange`` and refuses the same ones before any launch
    (descending segments were accepted until this module asked: a negative segment length in the kernel)."""
    from ibamd import backend as B
    part, dpart = rae_rank1
    loop = hl.fused_loop(part, 3).check()
    L = hl.LoopDevice(dev, loop)
    nc, v = dpart.nc, dev.vp
    rng = np.random.default_rng(41)
    uh = rng.uniform(-1, 1, nc).astype(np.float32)
    u, ud = ibamd.hip(uh), ibamd.hip(uh[::-1].copy())
    Cf, _, ldc = B._field(ibamd.hip(np.ones((nc, 2), dtype=np.float32)), nc)
    state = dev.state()
    fstate = torch.zeros(2, dtype=torch.int64, device=dev.dev)
    L.fill_bufs(hl.SENTINEL)
    down = dev.segs([0, 9, 5, loop.total])
    seg17, p17, fl17 = dev.segs([0] * 18), dev.ptrs([L.recv] * 17), dev.ptrs([L.flags] * 17)

    def step(send_all=L.send_all, ns=loop.K, sseg=L.sseg, dst=L.dst, sfl=L.sflags, nr=loop.K, rseg=L.rseg, rfl=L.rflags):
        return dev.call("ibh_step_advection_xgmi", dpart.handle, v(u), v(Cf), ldc, v(ud), v(send_all), ns, v(sseg),
                        v(dst[0]), v(dst[1]), v(sfl), v(L.recv_all), v(L.src[0]), v(L.src[1]), nr, v(rseg), v(rfl),
                        v(state), S, v(fstate))

    bad = [lambda: step(sseg=down), lambda: step(rseg=down), lambda: step(send_all=None), lambda: step(ns=0, nr=0),
           lambda: step(ns=17, sseg=seg17, dst=[p17, p17], sfl=fl17), lambda: step(nr=17, rseg=seg17, rfl=fl17)]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.IbhError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert np.array_equal(dev.words(u), uh.view(np.uint32))
    assert np.array_equal(dev.words(ud), uh[::-1].copy().view(np.uint32))
    assert np.all(L.read_bufs() == hl.SENTINEL) and np.all(L.read_flags() == 0)
    assert dev.words(state).tolist() == [0] * 8 and fstate.cpu().tolist() == [0, 0]
