"""The partitions the fused closures are checked on and the comparison they are held to: test infrastructure shared by
tests/test_gpu_les.py and tests/test_gpu_k_epsilon.py (each adds the fields of its own closure to ``Case`` by subclassing)."""
import numpy as np
import torch

import ibamd
import kepsilon_model as km
import les_model as lm
from ibamd import turbulence as T


class Case:
    def __init__(self, part):
        self.part = part
        self.dpart = ibamd.to_backend(part, ibamd.hip)
        self.nd = part.ndims
        self.nc = part.spacing.shape[0]

    def wavy(self, seed=21):
        """A velocity field with every gradient component alive, plus noise."""
        return km.wavy_velocity(self.part, seed)


def make_cases(case=Case):
    """Complete 8^3 blocks (wave per block), and block size 4: no block structure (thread per cell over the side table)."""
    out = {"octree": case(lm.one_partition(lm.octree_mesh())), "single": case(lm.one_partition(lm.single_block_mesh())),
           "bs4 2d": case(lm.one_partition(lm.bs4_mesh(2))), "bs4 3d": case(lm.one_partition(lm.bs4_mesh(3)))}
    for k in ("octree", "single"):
        assert T.all_blocks(out[k].dpart), k
    for k in ("bs4 2d", "bs4 3d"):
        d = out[k].dpart
        assert d.info["full_blocks"] == 0 and T.fused_closures_apply(d) and not T.all_blocks(d), k
        assert 0 < d.info["direct_sides"] < 2 * d.nd * d.nc, k     # some sides take the CSR walk (2:1 interfaces)
    return out


def assert_block_case(c, mesh):
    """The octree has a block count that is no multiple of the four waves of a workgroup; the single block stands alone."""
    i = c.dpart.info
    nblk = i["full_blocks"]
    assert nblk * 512 == c.nc
    if mesh == "octree":
        assert nblk % 4 != 0 and nblk > 4, nblk                  # the last workgroup has idle waves
        assert i["sides_fine"] > 0 and i["sides_coarse"] > 0
    else:
        assert nblk == 1


def grid_cap_case(case):
    """A face-list partition of just over 4096 * 256 cells: the launch is capped at 4096 workgroups."""
    f32 = np.float32
    msh = ibamd.Mesh(f32([0, 0]), f32([1, 1]), block_size=4,
                     refinement_regions=[(ibamd.Ball(np.array([0.5, 0.5]), 2.0), f32(1 / 1024)),
                                         (ibamd.Ball(np.array([0.3, 0.3]), 0.004), f32(1 / 2048))])
    c = case(lm.one_partition(msh))
    assert 4096 * 256 < c.nc < 4096 * 256 + 8192
    assert c.dpart.info["full_blocks"] == 0 and T.fused_closures_apply(c.dpart)
    return c


def skirt_case(case):
    """The second of two partitions of the octree: blocks and skirt fragments, not all-block -- the wrappers compose."""
    msh = lm.octree_mesh()
    dom = ibamd.Domain(msh, max_partition_size=-(-(-(-len(msh) // 2)) // 512) * 512, boundaries=False)
    assert len(dom.partitions) == 2
    c = case(dom.partitions[1])
    assert not T.fused_closures_apply(c.dpart) and c.dpart.info["full_blocks"] > 0
    return c


def adv2d_case(case, adv_mesh):
    """The 2-D advection mesh as one partition: 8^2 blocks, so the closures take the composed path."""
    (p,) = ibamd.Domain(adv_mesh, hypercube_families=[], boundaries=False, max_partition_size=10 ** 9).partitions.values()
    c = case(p)
    assert not T.fused_closures_apply(c.dpart)
    return c


def same(a, b):
    """Bit for bit where neither is NaN, and the same NaN pattern."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))
