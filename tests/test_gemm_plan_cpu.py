"""Which kernel a product runs on.  lrn_dbg_gemm_plan runs the launch planner of csrc/gemm_f64.hip for the descriptor
lrn_dbg_gemm would build and touches no device, so the dispatch is pinned here without a GPU: the GPU tests only see
numbers, and a product that slipped to a slower kernel would pass all of them.

The expected values were recorded from the dispatcher as it was before it became a planner (every launch of the old
gemm_impl written down by a stand-in for hipLaunchKernelGGL, profiles/gemm_refactor_ab.txt); none of them was produced
by the planner under test."""
import ctypes as C

import pytest

import loraine_jl_amd

REG64, REG128, LDS, MID, KSEG = 1, 2, 3, 4, 5
TRI_LOWER, KSEG_TRI = 1, 16

# (transA, transB, M, N, K, lda, ldb, ldc, beta, flags, ksplit) -> (kernel, tile, grid x, grid z, dynamic LDS, slabs)
ROWS = [
    # ---- shapes the GPU tests name (tests/test_gpu_blocks.py)
    # 128-tiles fill the chip (>= 256 of them), NT layout, K >= 256: direct-to-LDS kernel
    ((0, 1, 2048, 2048, 256, 2048, 2048, 2048, 0, 0, 1), (LDS, 128, 256, 1, 0, 1)),
    ((0, 1, 2000, 2176, 403, 2000, 2176, 2000, 0, 0, 1), (LDS, 128, 272, 1, 0, 1)),      # 16 x 17 tiles
    ((0, 1, 2050, 2300, 270, 2050, 2300, 2050, 0, 0, 1), (LDS, 128, 312, 1, 0, 1)),      # 17 x 18 tiles, odd ld
    # 256 .. 1023 128-tiles, square, plain: the round model prices the 64-tile DMA kernel cheaper
    ((0, 1, 2200, 2200, 2200, 2200, 2200, 2200, 0, 0, 1), (MID, 64, 1232, 1, 0, 1)),     # 35 x 35 = 1225 tiles, padded to 8
    ((0, 1, 3001, 3001, 3001, 3001, 3001, 3001, 0, 0, 1), (MID, 64, 2216, 1, 0, 1)),
    # fewer than 256 128-tiles, K >= 256, sides >= 128: split into slabs by the cost model, the slabs on the DMA kernel
    ((0, 1, 801, 801, 801, 801, 801, 801, 0, 0, 1), (MID, 64, 512, 1, 0, 3)),            # 169 tiles x 3 slabs = 507
    ((0, 1, 800, 800, 800, 800, 800, 800, 0, 0, 1), (MID, 64, 512, 1, 0, 3)),
    ((0, 1, 640, 640, 640, 640, 640, 640, 0, 0, 1), (MID, 64, 400, 1, 0, 4)),
    ((0, 1, 1111, 1111, 1111, 1111, 1111, 1111, 0, 0, 1), (MID, 64, 976, 1, 0, 3)),
    # test_gemm_mid_kernel_ragged_shapes: a side below 128 is never split, the others by the model
    ((0, 1, 10, 500, 100, 10, 500, 10, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 257, 513, 1000, 257, 513, 257, 0, 0, 1), (MID, 64, 184, 1, 0, 4)),
    ((0, 1, 64, 64, 64, 64, 64, 64, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 65, 63, 70, 65, 63, 65, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 1, 300, 64, 1, 300, 1, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 300, 1, 257, 300, 1, 300, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 129, 1100, 333, 129, 1100, 129, 0, 0, 1), (MID, 64, 168, 1, 0, 3)),
    # K < 64: the DMA pipeline has nothing to overlap, register-staged 64-tile kernel
    ((0, 1, 50, 50, 50, 50, 50, 50, 0, 0, 1), (REG64, 64, 8, 1, 0, 1)),
    # beta != 0 keeps an unsplit small product off the DMA kernel (it only stores) ...
    ((0, 1, 200, 136, 77, 200, 136, 200, 0.5, 0, 1), (REG64, 64, 16, 1, 0, 1)),
    ((0, 1, 50, 50, 50, 50, 50, 50, 0.5, 0, 1), (REG64, 64, 8, 1, 0, 1)),
    # ... a split one adds beta C in the slab reduction, and the direct-to-LDS kernel has the beta epilogue
    ((0, 1, 801, 801, 801, 801, 801, 801, 0.5, 0, 1), (MID, 64, 512, 1, 0, 3)),
    ((0, 1, 2048, 2048, 256, 2048, 2048, 2048, 0.5, 0, 1), (LDS, 128, 256, 1, 0, 1)),
    # an operand that is K-contiguous: register-staged kernels (grid z = the slabs of the split)
    ((1, 1, 200, 136, 77, 77, 136, 200, 0, 0, 1), (REG64, 64, 16, 1, 0, 1)),
    ((0, 0, 200, 136, 77, 200, 77, 200, 0, 0, 1), (REG64, 64, 16, 1, 0, 1)),
    ((1, 0, 200, 136, 77, 77, 77, 200, 0, 0, 1), (REG64, 64, 16, 1, 0, 1)),
    ((1, 1, 801, 801, 801, 801, 801, 801, 0, 0, 1), (REG64, 64, 176, 3, 0, 3)),
    ((0, 0, 801, 801, 801, 801, 801, 801, 0, 0, 1), (REG64, 64, 176, 3, 0, 3)),
    ((1, 0, 2048, 2048, 256, 256, 256, 2048, 0, 0, 1), (REG128, 128, 256, 1, 0, 1)),
    # GEMM_KSEG_TRI (test_gemm_packed_symmetric_dot): ld % 16 != 0 register-staged, ld % 16 == 0 K-contiguous DMA kernel
    ((1, 0, 200, 136, 300 * 300, 300 * 300, 300 * 300, 200, 0, KSEG_TRI, 4), (REG128, 128, 8, 4, 0, 1)),
    ((1, 0, 200, 136, 320 * 320, 320 * 320, 320 * 320, 200, 0, KSEG_TRI, 4), (KSEG, 128, 8, 4, 65536, 1)),
    # ---- borders
    # K = 63 / 64: the DMA kernel from 64 on
    ((0, 1, 700, 700, 63, 700, 700, 700, 0, 0, 1), (REG64, 64, 128, 1, 0, 1)),
    ((0, 1, 700, 700, 64, 700, 700, 700, 0, 0, 1), (MID, 64, 128, 1, 0, 1)),
    # K = 255 / 256: the direct-to-LDS kernel from 256 on
    ((0, 1, 2048, 2048, 255, 2048, 2048, 2048, 0, 0, 1), (REG128, 128, 256, 1, 0, 1)),
    ((0, 1, 2048, 2048, 256, 2048, 2048, 2048, 0, 0, 1), (LDS, 128, 256, 1, 0, 1)),
    # side 127 / 128: split from 128 on
    ((0, 1, 127, 127, 512, 127, 127, 127, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 128, 128, 512, 128, 128, 128, 0, 0, 1), (MID, 64, 16, 1, 0, 4)),
    # 255 / 256 128-tiles: the 64 tile below (15 x 17), the 128 tile from 256 on
    ((0, 1, 1920, 2176, 512, 1920, 2176, 1920, 0, 0, 1), (MID, 64, 1024, 1, 0, 1)),
    ((0, 1, 2048, 2048, 2048, 2048, 2048, 2048, 0, 0, 1), (LDS, 128, 256, 1, 0, 1)),     # (the round model prices the 128 tile cheaper)
    # 961 / 1024 128-tiles: the round model up to 1023 (here it prices the 128 tile cheaper), none from 1024 on
    ((0, 1, 3968, 3968, 3968, 3968, 3968, 3968, 0, 0, 1), (LDS, 128, 968, 1, 0, 1)),
    ((0, 1, 3969, 3969, 3969, 3969, 3969, 3969, 0, 0, 1), (LDS, 128, 1024, 1, 0, 1)),
    # no split below K = 256; a slab never shorter than 96: K = 287 allows 2 slabs, 288 three
    ((0, 1, 128, 128, 191, 128, 128, 128, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 128, 128, 192, 128, 128, 128, 0, 0, 1), (MID, 64, 8, 1, 0, 1)),
    ((0, 1, 128, 128, 287, 128, 128, 128, 0, 0, 1), (MID, 64, 8, 1, 0, 2)),
    ((0, 1, 128, 128, 288, 128, 128, 128, 0, 0, 1), (MID, 64, 16, 1, 0, 3)),
    # GEMM_TRI_LOWER alone: the lower 64-tiles as slabs, up to 6 of them (13 * 14 / 2 = 91 tiles x 5; 3 tiles x 2)
    ((0, 1, 801, 801, 801, 801, 801, 801, 0, TRI_LOWER, 1), (MID, 64, 456, 1, 0, 5)),
    ((0, 1, 129, 129, 256, 129, 129, 129, 0, TRI_LOWER, 1), (MID, 64, 16, 1, 0, 2)),
    # the caller's own split-K: its slabs on the DMA kernel (5 x 4 tiles x 7 = 140), no split of the planner's
    ((0, 1, 300, 200, 1000, 300, 200, 300, 0, 0, 7), (MID, 64, 144, 1, 0, 1)),
]


def _plan(args):
    lib = loraine_jl_amd.load_library()
    tA, tB, M, N, K, lda, ldb, ldc, beta, flags, ksplit = args
    out = (C.c_int * 6)()
    rc = lib.lrn_dbg_gemm_plan(tA, tB, M, N, K, lda, ldb, float(beta), ldc, flags, ksplit, out)
    return rc, tuple(out)


@pytest.mark.parametrize("args,expected", ROWS, ids=["-".join(str(a) for a in r[0]) for r in ROWS])
def test_gemm_plan(args, expected):
    rc, got = _plan(args)
    assert rc == 0
    assert got == expected


def test_gemm_plan_rejects_more_than_64_splits():
    rc, got = _plan((0, 1, 300, 200, 1000, 300, 200, 300, 0, 0, 65))
    assert rc == -1            # LRN_ERR_ARG
    assert got[0] == 0         # nothing planned


# ---- the shapes of tests/test_gpu_products.py
KFROM_N, KFROM_M, KTO_N, KTO_M, C_MIRROR, DYN_MASKS = 64, 128, 1024, 2048, 4096, 131072
K_RANGE_FLAG_SETS = [KFROM_M, KTO_M, KFROM_N, KTO_N, KFROM_N | TRI_LOWER | C_MIRROR, KTO_N | TRI_LOWER | C_MIRROR,
                     KFROM_M | TRI_LOWER]


@pytest.mark.parametrize("dyn", [0, DYN_MASKS])
@pytest.mark.parametrize("flags", K_RANGE_FLAG_SETS)
@pytest.mark.parametrize("n,kernel", [(300, LDS), (385, LDS), (400, LDS), (130, REG128)])
def test_k_range_products_take_the_128_tile(n, kernel, flags, dyn):
    """Any K-range flag forces the 128 tile whatever the size: the direct-to-LDS kernel from K = 256 on, below it the
    register-staged one with its own K-range code -- the GPU file covers both."""
    rc, got = _plan((0, 1, n, n, n, n, n, n, 0, flags | dyn, 1))
    assert rc == 0
    assert got[:2] == (kernel, 128)
    assert got[5] == 1


@pytest.mark.parametrize("flags", [KFROM_M, KTO_M, KFROM_M | DYN_MASKS, KTO_M | DYN_MASKS])
def test_k_range_rectangular_product_takes_the_128_tile(flags):
    rc, got = _plan((0, 1, 300, 140, 300, 300, 140, 300, 0, flags, 1))
    assert rc == 0
    assert got[:2] == (LDS, 128)


# split factor of a square NT product of side n: (lower 64-tiles alone, full product) -- auto_split_factor restated by hand
SPLIT_FACTORS = {255: (1, 1), 256: (2, 2), 300: (3, 3), 385: (4, 4), 481: (5, 4), 650: (6, 4), 1100: (4, 3), 1300: (2, 1)}


@pytest.mark.parametrize("n", sorted(SPLIT_FACTORS))
def test_split_factors_of_the_product_layer_sizes(n):
    got = []
    for flags in (TRI_LOWER, 0):
        rc, plan = _plan((0, 1, n, n, n, n, n, n, 0.0, flags, 1))
        assert rc == 0
        got.append(plan[5])
    assert tuple(got) == SPLIT_FACTORS[n]


def test_split_factors_cover_every_value():
    assert {v[0] for v in SPLIT_FACTORS.values()} == {1, 2, 3, 4, 5, 6}
    assert {v[1] for v in SPLIT_FACTORS.values()} == {1, 2, 3, 4}
