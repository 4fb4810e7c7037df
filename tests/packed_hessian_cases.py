"""What the tests of the packed dense Hessians share (hqpkkt_set_packed_hessians; test_staged_packed_hessian_cpu.py,
test_gpu_staged_packed_hessian.py): the layout rule in numpy and the stage sizes at the edges of the 128-wide tile."""
import numpy as np

from dense_hessian_cases import up8

T = 128
COPY_ROWS = 64  # a host block's rows are moved in groups of 64, every group from its first column on
# block orders at the edges of the rule: 312 does not pack, 313 does; 384 packs, 385 does not; 401 does not, 402 does
ORDERS = (312, 313, 384, 385, 401, 402, 640)


def tiles(nz):
    nt = -(-nz // T)
    return nt * (nt + 1) // 2


def packs(nz):
    return tiles(nz) * T * T < nz * up8(nz)


def arena(nz):
    """Doubles a stage takes with packing asked for."""
    return tiles(nz) * T * T if packs(nz) else nz * up8(nz)


def handover(nz):
    """Doubles one dense hand-over of a host block moves."""
    if not packs(nz):
        return nz * nz
    return sum(min(COPY_ROWS, nz - r) * (nz - r) for r in range(0, nz, COPY_ROWS))


def scratch(nz):
    """Doubles of the product's scratch: per row tile r a slot of T doubles per 8 tiles of its own row and one per tile below it."""
    nt = -(-nz // T)
    return sum(-(-(r + 1) // 8) + nt - 1 - r for r in range(nt)) * T if packs(nz) else 0


def rows_of(orders):
    """hessian_packing() as the rule gives it."""
    return np.array([[T if packs(nz) else 0, tiles(nz) if packs(nz) else 0, arena(nz), handover(nz), scratch(nz)] for nz in orders], dtype=np.int64)


def one_stage(nz, nu=2, nk=5):
    """Stage sizes (nx, nu) of K = 1 with a first stage of order nz and a small terminal stage."""
    return [nz - nu, nk], [nu]
