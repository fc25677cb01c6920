"""The numpy model of the direct halo exchange (tests/halo_loopback.py) is the reference of
tests/test_gpu_halo_loopback.py, so it is pinned first, without a GPU: on the real plans of cut meshes it must reproduce
the reference's per-call gather (every rank's array equals ``global[part.domain]``), each of its four conventions must
matter, and the self-loop tables of the device module must be well formed."""
import numpy as np
import pytest

import halo_loopback as hl
from conftest import advection_mesh, rae_mesh

CUTS = [("adv", 3), ("adv", 4), ("adv", 8), ("rae", 8)]
NVS = (1, 5)


@pytest.fixture(scope="module")
def cuts():
    meshes = {"adv": advection_mesh(2e-2), "rae": rae_mesh()}
    return {(m, w): (len(meshes[m]),) + hl.real_plans(meshes[m], w) for m, w in CUTS}


def _two_rounds(ncells, dom, plans, nv, model=None, oversize=False):
    """Two rounds (parity 0, then 1; the owners' values change in between) on poisoned skirts: True iff after each round
    every rank's storage equals ``global[part.domain]`` as bits, padding included."""
    rng = np.random.default_rng(4321 + nv)
    bufs = None
    if oversize:   # room for blocks at wrong offsets: a planted error must show as wrong values, not as a numpy error
        words = nv * max(max(p.n_send, p.n_recv) for p in plans.values())
        bufs = {p: np.zeros((2, words), dtype=np.uint32) for p in plans}
    ok = True
    for rnd in (0, 1):
        G = rng.integers(0, 2 ** 32, size=(nv, ncells), dtype=np.uint64).astype(np.uint32)
        lds = {p: plans[p].nc + (5 if p % 2 else 0) for p in plans}
        fields = {p: hl.rank_storage(G, dom.partitions[p], nv, lds[p]) for p in plans}
        bufs = hl.model_exchange(plans, fields, nv, rnd & 1, bufs, model=model)
        ok = ok and all(np.array_equal(fields[p], hl.expected_storage(G, dom.partitions[p], nv, lds[p])) for p in plans)
    return ok


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("cut", CUTS, ids=lambda c: f"{c[0]}{c[1]}")
def test_real_plans_reproduce_the_global_field(cuts, cut, nv):
    ncells, dom, plans = cuts[cut]
    for p in plans:
        skirt = dom.partitions[p].domain.shape[0] - dom.partitions[p].image.size
        assert skirt > 0 and plans[p].n_recv == skirt
    assert _two_rounds(ncells, dom, plans, nv)


def test_peer_counts_and_symmetry(cuts):
    """The shapes the device module rests on: up to 7 peers per rank, never fewer than 3 on the cuts it runs."""
    for (m, w), (_, dom, plans) in cuts.items():
        for p, plan in plans.items():
            assert sorted(plan.send) == sorted(plan.recv) == plan.peers, (m, w, p)
            for q in plan.peers:
                assert plan.send[q].size == plans[q].recv[p].size > 0, (m, w, p, q)
    rae = [len(p.peers) for p in cuts[("rae", 8)][2].values()]
    assert max(rae) >= 7 and min(rae) >= 3, rae
    assert [len(p.peers) for p in cuts[("adv", 4)][2].values()] == [3, 3, 3, 3]
    assert cuts[("rae", 8)][0] == 37120


# ---- the model has teeth: each convention, broken in a copy, breaks the equality on a real plan
class SenderOrder(hl.Model):
    def block_offset(self, plans, sender, receiver, nv):
        off = 0
        for q in sorted(plans[sender].send):       # the SENDER's peer order
            if q == receiver:
                return off
            off += nv * int(plans[sender].send[q].size)


class RowMajor(hl.Model):
    def pack(self, field, rows, nv):
        return field[:nv, rows].T.reshape(-1)      # element (i, v) at i*nv + v


class OtherParity(hl.Model):
    def read_parity(self, parity):
        return 1 - parity


class SegOffByOne(hl.Model):
    def seg_of(self, seg, t):
        return np.searchsorted(seg[1:-1], t, side="left")   # t > seg[q+1] where t >= seg[q+1] is meant


def _breaks(cuts, model):
    return [(cut, nv) for cut in CUTS for nv in NVS if not _two_rounds(*cuts[cut], nv, model=model(), oversize=True)]


def test_oversized_buffers_do_not_change_the_model(cuts):
    assert _breaks(cuts, hl.Model) == []


def test_planted_sender_peer_order_is_seen(cuts):
    assert _breaks(cuts, SenderOrder)


def test_planted_row_major_block_is_seen(cuts):
    broken = _breaks(cuts, RowMajor)
    assert broken and all(nv > 1 for _, nv in broken)     # one variable has one layout


def test_planted_other_parity_is_seen(cuts):
    assert len(_breaks(cuts, OtherParity)) == len(CUTS) * len(NVS)


def test_planted_seg_of_off_by_one_is_seen(cuts):
    broken = _breaks(cuts, SegOffByOne)
    assert broken and all(nv > 1 for _, nv in broken)     # with one variable the neighbouring block starts at the same word


# ---- the tables of the device module
def test_exchange_case_list_covers_what_the_issue_names():
    segs = {tuple(c[1]) for c in hl.EXCHANGE_CASES}
    for s in ([257], [1], [100, 0, 57], [0, 64, 0], [0, 0, 0], hl.SIXTEEN, [16384 + 3], [9000, 0, 7387 + 3]):
        assert tuple(s) in segs
    assert len(hl.SIXTEEN) == 16 and min(hl.SIXTEEN) == 0 and max(hl.SIXTEEN) == 40
    assert {c[3] for c in hl.EXCHANGE_CASES} == {1, 2, 3, 5, 7} and {c[4] for c in hl.EXCHANGE_CASES} == {0, 5}
    for s in ([16384 + 3], [9000, 0, 7387 + 3]):
        assert {(c[3], c[4]) for c in hl.EXCHANGE_CASES if c[1] == s} == {(1, 0), (1, 5), (5, 0), (5, 5)}
    assert any(c[2] != list(range(len(c[2]))) for c in hl.EXCHANGE_CASES)
    assert len({c[0] for c in hl.EXCHANGE_CASES}) == len(hl.EXCHANGE_CASES)


@pytest.mark.parametrize("case", hl.EXCHANGE_CASES + [("timeout",) + tuple(hl.TIMEOUT_LOOP.values()),
                                                      ("graph",) + tuple(hl.GRAPH_LOOP.values()),
                                                      ("argcheck",) + tuple(hl.ARGCHECK_LOOP.values())],
                         ids=lambda c: c[0])
def test_self_loop_tables_are_well_formed(case):
    _, seg, perm, nv, pad = case
    loop = hl.exchange_loop(seg, perm, nv, pad).check()
    assert loop.ld == loop.n + pad and loop.total == sum(seg)
    # the model through the buffers and the direct statement of the effect agree, and touch nothing else
    rng = np.random.default_rng(3)
    f = rng.integers(0, 2 ** 32, size=(nv, loop.ld), dtype=np.uint64).astype(np.uint32)
    bufs = np.full((2, loop.buf_words), hl.SENTINEL, dtype=np.uint32)
    want = loop.expected(f)
    got = loop.model(f.copy(), bufs, 1)
    assert np.array_equal(got, want)
    assert np.all(bufs[0] == hl.SENTINEL)
    untouched = np.ones(loop.ld, dtype=bool)
    untouched[loop.recv_all] = False
    assert np.array_equal(want[:, untouched], f[:, untouched])
    if loop.total:
        assert not np.array_equal(want, f)


@pytest.mark.parametrize("K", [1, 3, 16])
def test_fused_self_loop_tables_are_well_formed(K):
    import ibamd
    msh = rae_mesh()
    dom = ibamd.Domain(msh, max_partition_size=hl.partition_size(len(msh), 2), boundaries=False, only=[1])
    part = dom.partitions[1]
    loop = hl.fused_loop(part, K).check()
    skirt = np.ones(part.domain.shape[0], dtype=bool)
    skirt[part.image_in_domain] = False
    assert loop.K == K and loop.total == int(skirt.sum()) > 0
    assert np.array_equal(np.sort(loop.recv_all), np.nonzero(skirt)[0])
    assert not skirt[loop.send_all].any()
    if K > 1:
        assert 0 in np.diff(loop.rseg) and loop.perm.tolist() != list(range(K))


def test_synthetic_two_rank_plan_is_a_mirror():
    plans = hl.synthetic_two_rank_plans(65536 + 3, 5, seed=5)
    assert plans[1].send[2].size == plans[2].recv[1].size == 65536 + 3
    assert plans[2].send[1].size == plans[1].recv[2].size == 5
    for p in plans.values():
        rows = np.concatenate(list(p.send.values()) + list(p.recv.values()))
        assert np.unique(rows).size == rows.size and rows.min() >= 0 and rows.max() < p.nc
