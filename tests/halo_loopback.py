"""Tables and numpy model for running the direct xGMI halo kernels in ONE process (no torch.distributed).

The kernels of csrc/ibh_halo.hip, csrc/ibh_halo_dev.h and the exchange part of ``k_step_quad`` only see pointers, so one
process can own the buffers of every rank: either W ranks side by side (``RankSet``: push for every rank, then pull for
every rank, on one stream), or one rank that is its own K peers (``SelfLoop``).  The reference is a numpy gather and
scatter on ``uint32`` storages, compared as raw bits (NaN payloads, -0.0, Inf and denormals survive).

Fields are ``(nv, ld)`` storages: variable ``v`` of row ``c`` is ``field[v, c]``, what the kernels address as
``f[c + v*ld]``; columns ``n..ld`` are padding that no exchange may touch.
"""
import numpy as np

SENTINEL = np.uint32(0x5E471E15)   # what the receive buffers hold before anything was pushed
POISON = np.uint32(0x7FC0DEAD)     # a NaN payload: stale skirt rows
PAD = np.uint32(0xFFA5A5A5)        # another one: the padding columns n..ld
MAX_SPINS = 256                    # bound of every wait of the device module (a protocol error is a status bit, not a spin)


# ---------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------
class Plan:
    """The part of ``ibamd.halo.HaloPlan`` the model reads: ``send[q]`` / ``recv[q]`` = local rows per peer, ``nc`` rows."""

    def __init__(self, nc, send, recv):
        self.nc = int(nc)
        self.send = {int(q): np.asarray(v, dtype=np.int32) for q, v in send.items()}
        self.recv = {int(q): np.asarray(v, dtype=np.int32) for q, v in recv.items()}


def partition_size(ncells, world):
    """``max_partition_size`` of a cut in ``world`` parts (as tests/test_halo_gloo.py)."""
    return -(-(-(-ncells // world)) // 64) * 64


def real_plans(msh, world):
    """``(dom, {pid: HaloPlan})`` of ``msh`` cut in ``world`` partitions."""
    import ibamd
    from ibamd.halo import HaloPlan
    dom = ibamd.Domain(msh, max_partition_size=partition_size(len(msh), world), boundaries=False)
    assert len(dom.partitions) == world
    return dom, {p: HaloPlan(dom, p) for p in sorted(dom.partitions)}


def synthetic_two_rank_plans(n_big, n_small, seed):
    """Two ranks: rank 1 sends ``n_big`` rows to rank 2 and receives ``n_small``; rows random, unsorted, disjoint."""
    rng = np.random.default_rng(seed)
    n1, n2 = n_big + n_small + 11, n_big + n_small + 7
    r1, r2 = rng.permutation(n1), rng.permutation(n2)
    p1 = Plan(n1, {2: r1[:n_big]}, {2: r1[n_big:n_big + n_small]})
    p2 = Plan(n2, {1: r2[:n_small]}, {1: r2[n_small:n_small + n_big]})
    return {1: p1, 2: p2}


def recv_layout(plan, nv):
    """``({peer: word offset of its block}, words per parity)`` of the receive buffer of ``plan``: the blocks of the sorted
    receive peers back to back."""
    off, o = {}, 0
    for q in sorted(plan.recv):
        off[q] = o
        o += nv * int(plan.recv[q].size)
    return off, o


def rank_storage(G, part, nv, ld, poison=True):
    """``(nv, ld)`` storage of a rank holding ``G[:, part.domain]``; skirt rows poisoned, padding columns ``PAD``."""
    nc = part.domain.shape[0]
    a = np.full((nv, ld), PAD, dtype=np.uint32)
    a[:, :nc] = G[:nv, np.asarray(part.domain)]
    if poison:
        skirt = np.ones(nc, dtype=bool)
        skirt[part.image_in_domain] = False
        a[:, :nc][:, skirt] = POISON
    return a


def expected_storage(G, part, nv, ld):
    return rank_storage(G, part, nv, ld, poison=False)


# ---------------------------------------------------------------------------------------------------------------------
# the model: include/ibhip.h, "The whole exchange in two launches", word by word
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """The four conventions of the exchange, one method each (tests/test_halo_loopback_model.py plants an error in each
    and checks that the model then no longer reproduces the global field)."""

    def block_offset(self, plans, sender, receiver, nv):
        # "src (the peers' blocks back to back ...)": the offset of the sender among the RECEIVER's sorted receive peers
        return recv_layout(plans[receiver], nv)[0][sender]

    def pack(self, field, rows, nv):
        # "(n_q, nv) column-major": element (i, v) at i + v*n_q
        return field[:nv, rows].reshape(-1)

    def read_parity(self, parity):
        return parity

    def seg_of(self, seg, t):
        # the peer whose segment seg[q] .. seg[q+1] holds t (empty segments hold nothing)
        return np.searchsorted(seg[1:-1], t, side="right")


def model_exchange(plans, fields, nv, parity, bufs=None, push=True, pull=True, model=None):
    """One exchange among the ranks of ``plans`` (``{pid: plan}``) on ``fields`` (``{pid: (nv, ld) uint32}``, changed in
    place).  ``bufs[pid]`` = the receive buffer of the rank, ``(2, words)`` for the two parities (made of zeros when not
    given); returned.  ``push`` / ``pull``: only that half."""
    model = model or Model()
    if bufs is None:
        bufs = {p: np.zeros((2, max(recv_layout(plans[p], nv)[1], 1)), dtype=np.uint32) for p in plans}
    if push:
        for r in sorted(plans):
            for q in sorted(plans[r].send):                    # every peer in ascending order
                rows = plans[r].send[q]
                assert rows.size == plans[q].recv[r].size
                o = model.block_offset(plans, r, q, nv)
                bufs[q][parity, o:o + nv * rows.size] = model.pack(fields[r], rows, nv)
    if pull:
        for r in sorted(plans):
            peers = sorted(plans[r].recv)
            if not peers:
                continue
            recv_all = np.concatenate([plans[r].recv[q] for q in peers])
            seg = np.concatenate([[0], np.cumsum([plans[r].recv[q].size for q in peers])]).astype(np.int64)
            src = bufs[r][model.read_parity(parity)]
            t = np.arange(seg[-1])
            q = model.seg_of(seg, t)
            i, nq = t - seg[q], seg[q + 1] - seg[q]
            for v in range(nv):
                fields[r][v, recv_all] = src[seg[q] * nv + i + v * nq]
    return bufs


# ---------------------------------------------------------------------------------------------------------------------
# one rank as its own K peers
# ---------------------------------------------------------------------------------------------------------------------
class SelfLoop:
    """Tables that make one rank its own ``K = len(seg_sizes)`` peers.  ``seg_sizes`` are the RECEIVE segments; send peer
    ``q`` lands in receive slot ``perm[q]`` (so send segment ``q`` has ``seg_sizes[perm[q]]`` rows, its block goes to word
    ``rseg[perm[q]]*nv`` of the parity buffer, and flag slot ``perm[q]`` is its flag).  Send and receive rows are disjoint,
    random and unsorted; ``recv_rows`` / ``send_pool`` fix the set of receive rows and the set the send rows are drawn
    from (the fused step: skirt rows and image rows)."""

    def __init__(self, n_rows, seg_sizes, perm, nv, ld, seed, recv_rows=None, send_pool=None):
        self.n, self.nv, self.ld = int(n_rows), int(nv), int(ld)
        self.K = len(seg_sizes)
        self.perm = np.asarray(perm, dtype=np.int64)
        rsz = np.asarray(seg_sizes, dtype=np.int64)
        ssz = rsz[self.perm] if self.K else rsz
        self.rseg = np.concatenate([[0], np.cumsum(rsz)]).astype(np.int64)
        self.sseg = np.concatenate([[0], np.cumsum(ssz)]).astype(np.int64)
        self.total = int(self.rseg[-1])
        rng = np.random.default_rng(seed)
        if recv_rows is None:
            draw = rng.permutation(self.n)[:2 * self.total]
            self.send_all, self.recv_all = draw[:self.total].astype(np.int32), draw[self.total:].astype(np.int32)
        else:
            self.recv_all = rng.permutation(np.asarray(recv_rows)).astype(np.int32)
            self.send_all = rng.choice(np.asarray(send_pool), self.total, replace=False).astype(np.int32)
        self.buf_words = max(self.total * self.nv, 1)     # per parity

    def dst_word(self, q, parity):
        """Word of the two-parity receive buffer at which the block of send peer ``q`` starts."""
        return parity * self.buf_words + int(self.rseg[self.perm[q]]) * self.nv

    def check(self):
        """Well-formedness: what a launch needs to stay inside its arrays."""
        assert sorted(self.perm.tolist()) == list(range(self.K)) and 0 <= self.K
        assert self.ld >= self.n and self.nv >= 1
        assert self.send_all.size == self.recv_all.size == self.total == int(self.sseg[-1])
        both = np.concatenate([self.send_all, self.recv_all])
        assert np.unique(both).size == both.size, "send and receive rows must be disjoint and unique"
        assert both.size == 0 or (both.min() >= 0 and both.max() < self.n)
        assert np.all(np.diff(self.rseg) >= 0) and np.all(np.diff(self.sseg) >= 0)
        covered = np.zeros(self.buf_words, dtype=np.int32)
        for q in range(self.K):
            nq = int(self.sseg[q + 1] - self.sseg[q])
            assert nq == int(self.rseg[self.perm[q] + 1] - self.rseg[self.perm[q]])
            for par in (0, 1):
                w = self.dst_word(q, par)
                assert par * self.buf_words <= w and w + nq * self.nv <= (par + 1) * self.buf_words
            w = self.dst_word(q, 0)
            covered[w:w + nq * self.nv] += 1
        assert self.total == 0 or np.all(covered == 1), "the blocks tile the parity buffer"
        return self

    def expected(self, f_old):
        """f_new[recv_all[rseg[perm[q]] + i], v] = f_old[send_all[sseg[q] + i], v]; every other word unchanged."""
        f = f_old.copy()
        for q in range(self.K):
            k = int(self.perm[q])
            i = np.arange(int(self.sseg[q + 1] - self.sseg[q]))
            f[:self.nv, self.recv_all[self.rseg[k] + i]] = f_old[:self.nv, self.send_all[self.sseg[q] + i]]
        return f

    def model(self, field, bufs, parity, push=True, pull=True):
        """The exchange through the buffers: ``field`` (``(nv, ld)``) and ``bufs`` (``(2, buf_words)``) change in place."""
        nv = self.nv
        if push:
            for q in range(self.K):
                rows = self.send_all[self.sseg[q]:self.sseg[q + 1]]
                w = self.dst_word(q, 0)
                bufs[parity, w:w + nv * rows.size] = field[:nv, rows].reshape(-1)
        if pull:
            for k in range(self.K):
                rows = self.recv_all[self.rseg[k]:self.rseg[k + 1]]
                w = int(self.rseg[k]) * nv
                field[:nv, rows] = bufs[parity, w:w + nv * rows.size].reshape(nv, rows.size)
        return field


def rotation(K, a=1, b=2):
    """A permutation of ``range(K)`` without fixed points for K = 3 (a=1, b=2) and K = 16 (a=3, b=5)."""
    return [(q * a + b) % K for q in range(K)]


SIXTEEN = [0, 40, 1, 0, 17, 33, 0, 0, 5, 40, 2, 29, 0, 11, 38, 0]


def _exchange_cases():
    """(id, seg_sizes, perm, nv, pad) of tests/test_gpu_halo_loopback.py::test_exchange_self_loop; pad: ld = n + pad."""
    out = []
    small = [("one257", [257]), ("one1", [1]), ("mid_empty", [100, 0, 57]), ("ends_empty", [0, 64, 0]),
             ("all_empty", [0, 0, 0]), ("sixteen", SIXTEEN)]
    for name, seg in small:
        K = len(seg)
        perms = [("id", list(range(K)))]
        if K == 3:
            perms.append(("rot", rotation(3)))
        if K == 16:
            perms.append(("rot", rotation(16, 3, 5)))
        for pname, perm in perms:
            for nv in (1, 2, 3, 5, 7):
                for pad in (0, 5):
                    # the identity is the plain case: trimmed to two variable counts where a permutation exists
                    if K > 1 and pname == "id" and not (nv in (1, 3) and pad == 5):
                        continue
                    out.append((f"{name}-{pname}-nv{nv}-pad{pad}", seg, perm, nv, pad))
    # totals past the cap of 64 workgroups x 256 threads: the second trip of the grid-stride loops
    big = [("cap_plus3", [16384 + 3], [0]), ("cap_three", [9000, 0, 7387 + 3], rotation(3)),
           ("cap_boundary_in_trip2", [16384 + 2, 0, 5], rotation(3))]
    for name, seg, perm in big:
        for nv in (1, 5):
            for pad in (0, 5):
                out.append((f"{name}-nv{nv}-pad{pad}", seg, perm, nv, pad))
    return out


EXCHANGE_CASES = _exchange_cases()


def exchange_loop(seg, perm, nv, pad, seed=7):
    n = 2 * int(sum(seg)) + 37
    return SelfLoop(n, seg, perm, nv, n + pad, seed)


TIMEOUT_LOOP = dict(seg=[40, 0, 23], perm=rotation(3), nv=2, pad=5)   # the three-peer loop of the time-out test
GRAPH_LOOP = dict(seg=[70, 0, 31], perm=rotation(3), nv=3, pad=5)     # the three-segment loop of the graph test
ARGCHECK_LOOP = dict(seg=[9, 4, 6], perm=rotation(3), nv=2, pad=5)

FUSED_WEIGHTS = [0, 3, 1, 0, 2, 5, 0, 0, 1, 4, 2, 3, 0, 1, 6, 0]


def split_sizes(total, K):
    """``total`` rows in 1, 3 or 16 segments, some of them empty."""
    if K == 1:
        return [total]
    if K == 3:
        return [total // 2, 0, total - total // 2]
    assert K == 16
    s = [total * w // sum(FUSED_WEIGHTS) for w in FUSED_WEIGHTS]
    s[14] += total - sum(s)
    return s


def fused_loop(part, K, seed=11):
    """Self-loop of the fused step on ``part``: receive rows = all skirt rows, send rows = as many image rows."""
    nc = part.domain.shape[0]
    skirt = np.ones(nc, dtype=bool)
    skirt[part.image_in_domain] = False
    rows = np.nonzero(skirt)[0]
    perm = list(range(K)) if K == 1 else rotation(3) if K == 3 else rotation(16, 3, 5)
    return SelfLoop(nc, split_sizes(rows.size, K), perm, 1, nc, seed, recv_rows=rows,
                    send_pool=np.asarray(part.image_in_domain))


# ---------------------------------------------------------------------------------------------------------------------
# device side (imported by the GPU module only)
# ---------------------------------------------------------------------------------------------------------------------
class Device:
    """Fine-grained allocations (``ibh_ipc_alloc(..., 1)``: the production memory kind) and raw library calls on torch's
    current stream.  ``close`` frees everything (fixture finaliser)."""

    def __init__(self):
        import ctypes
        import torch
        from ibamd import backend as B
        self.C, self.B, self.torch = ctypes, B, torch
        self.dev = B._dev()
        self._ptrs = []

    def alloc(self, words):
        p = self.B.c_vp()
        self.B.call("ibh_ipc_alloc", self.C.byref(p), 4 * max(int(words), 1), 1)
        self._ptrs.append(p)
        return int(p.value)

    def close(self):
        self.torch.cuda.synchronize()
        for p in self._ptrs:
            self.B.call("ibh_ipc_free", p)
        self._ptrs = []

    def call(self, name, *args):
        self.B._stream()          # as the product wrappers do before a raw call
        return self.B.call(name, *args)

    def write(self, addr, words):
        a = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        self.call("ibh_h2d", self.B.c_vp(addr), a.ctypes.data_as(self.B.c_vp), a.nbytes)

    def read(self, addr, n):
        a = np.empty(int(n), dtype=np.uint32)
        self.call("ibh_d2h", a.ctypes.data_as(self.B.c_vp), self.B.c_vp(addr), a.nbytes)
        return a

    def tensor(self, a):
        """Device tensor holding the words of ``a`` (uint32 / int32 / float32 array)."""
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(a.copy()).to(self.dev)

    def upload(self, t, a):
        """New contents for the device tensor ``t`` (same shape)."""
        t.copy_(self.tensor(a))

    def words(self, t):
        """Host copy of a device tensor as uint32."""
        return t.detach().cpu().numpy().view(np.uint32)

    def state(self):
        return self.torch.zeros(8, dtype=self.torch.int32, device=self.dev)

    def ptrs(self, addrs):
        return (self.C.c_void_p * max(len(addrs), 1))(*[int(a) for a in addrs])

    def segs(self, seg):
        return (self.C.c_int32 * len(seg))(*[int(s) for s in seg])

    def vp(self, x):
        """c_void_p of a tensor, a ctypes array, an address or None."""
        B, C = self.B, self.C
        if x is None:
            return B.c_vp(None)
        if isinstance(x, self.torch.Tensor):
            return B.c_vp(x.data_ptr())
        if isinstance(x, int):
            return B.c_vp(x)
        return C.cast(x, B.c_vp)


class LoopDevice:
    """Device tables of a ``SelfLoop``: two-parity receive buffer and K flag words (fine-grained), index lists, and the
    host-side launch tables as ``XgmiHalo._device_tables`` builds them."""

    def __init__(self, dev, loop):
        self.dev, self.loop = dev, loop
        K = loop.K
        self.recv = dev.alloc(2 * loop.buf_words)
        self.flags = dev.alloc(max(K, 1))
        # (a one-word list stands in for an empty one: the entry points want non-null pointers)
        self.send_all = dev.tensor(loop.send_all if loop.total else np.zeros(1, np.int32))
        self.recv_all = dev.tensor(loop.recv_all if loop.total else np.zeros(1, np.int32))
        self.sseg, self.rseg = dev.segs(loop.sseg), dev.segs(loop.rseg)
        self.dst = [dev.ptrs([self.recv + 4 * loop.dst_word(q, par) for q in range(K)]) for par in (0, 1)]
        self.sflags = dev.ptrs([self.flags + 4 * int(loop.perm[q]) for q in range(K)])
        self.rflags = dev.ptrs([self.flags + 4 * k for k in range(K)])
        self.src = [self.recv, self.recv + 4 * loop.buf_words]

    def fill_bufs(self, word):
        self.dev.write(self.recv, np.full(2 * self.loop.buf_words, word, dtype=np.uint32))

    def read_bufs(self):
        return self.dev.read(self.recv, 2 * self.loop.buf_words).reshape(2, self.loop.buf_words)

    def read_flags(self):
        return self.dev.read(self.flags, max(self.loop.K, 1))

    def exchange_args(self, state, max_spins):
        v, K = self.dev.vp, self.loop.K
        return (v(self.send_all), K, v(self.sseg), v(self.dst[0]), v(self.dst[1]), v(self.sflags), v(self.recv_all),
                v(self.src[0]), v(self.src[1]), K, v(self.rseg), v(self.rflags), v(state), int(max_spins))

    def exchange(self, field, state, max_spins=MAX_SPINS):
        v = self.dev.vp
        self.dev.call("ibh_halo_exchange", v(field), self.loop.nv, self.loop.ld, *self.exchange_args(state, max_spins))

    def push(self, field, state, parity):
        v = self.dev.vp
        self.dev.call("ibh_halo_push", v(field), self.loop.nv, self.loop.ld, v(self.send_all), self.loop.K, v(self.sseg),
                      v(self.dst[parity]), v(self.sflags), v(state))

    def pull(self, field, state, parity, max_spins=MAX_SPINS):
        v = self.dev.vp
        self.dev.call("ibh_halo_pull", v(field), self.loop.nv, self.loop.ld, v(self.recv_all), v(self.src[parity]),
                      self.loop.K, v(self.rseg), v(self.rflags), v(state), int(max_spins))


class RankSet:
    """W ranks in one process: every rank has its own two-parity receive buffer, W flag words and state words.
    ``push(r, field, parity)`` writes into the peers' buffers at the offset of ``r`` within each peer and signals slot
    ``r - 1`` of the peers' flag arrays; ``pull(r, field, parity)`` waits on slots ``q - 1`` of its own flag array."""

    def __init__(self, dev, plans, nv, lds):
        self.dev, self.plans, self.nv, self.lds = dev, plans, nv, lds
        W = max(plans)
        self.off, self.size, self.recv, self.flags, self.state, self.tab = {}, {}, {}, {}, {}, {}
        for r, plan in plans.items():
            self.off[r], n = recv_layout(plan, nv)
            self.size[r] = max(n, 1)
            self.recv[r] = dev.alloc(2 * self.size[r])
            self.flags[r] = dev.alloc(W)
            self.state[r] = dev.state()
        for r, plan in plans.items():
            sp, rp = sorted(plan.send), sorted(plan.recv)
            t = dict(sp=sp, rp=rp)
            t["send_all"] = dev.tensor(np.concatenate([plan.send[q] for q in sp]))
            t["recv_all"] = dev.tensor(np.concatenate([plan.recv[q] for q in rp]))
            t["sseg"] = dev.segs(np.concatenate([[0], np.cumsum([plan.send[q].size for q in sp])]))
            t["rseg"] = dev.segs(np.concatenate([[0], np.cumsum([plan.recv[q].size for q in rp])]))
            t["dst"] = [dev.ptrs([self.recv[q] + 4 * (par * self.size[q] + self.off[q][r]) for q in sp]) for par in (0, 1)]
            t["sflags"] = dev.ptrs([self.flags[q] + 4 * (r - 1) for q in sp])
            t["rflags"] = dev.ptrs([self.flags[r] + 4 * (q - 1) for q in rp])
            self.tab[r] = t

    def push(self, r, field, parity):
        v, t = self.dev.vp, self.tab[r]
        self.dev.call("ibh_halo_push", v(field), self.nv, self.lds[r], v(t["send_all"]), len(t["sp"]), v(t["sseg"]),
                      v(t["dst"][parity]), v(t["sflags"]), v(self.state[r]))

    def pull(self, r, field, parity, max_spins=MAX_SPINS):
        v, t = self.dev.vp, self.tab[r]
        self.dev.call("ibh_halo_pull", v(field), self.nv, self.lds[r], v(t["recv_all"]),
                      v(self.recv[r] + 4 * parity * self.size[r]), len(t["rp"]), v(t["rseg"]), v(t["rflags"]),
                      v(self.state[r]), int(max_spins))

    def read_bufs(self, r):
        return self.dev.read(self.recv[r], 2 * self.size[r]).reshape(2, self.size[r])
