"""CPU: the integer arithmetic by which the persistent NT GEMM shares out its remainder round by K range (csrc/gemm_plan.h: nt_stream_k
on the host, stream_k_items at the top of gemm_bf16_nt256_kernel<MODE, SK = true> on the device), queried from the library itself
(hct_gemm_describe, hct_gemm_stream_k_items: host arithmetic, no device call) and checked for every tile count, K and grid the host
rule admits: each remainder tile is covered exactly once by contiguous pieces of at least two stage pairs, its first piece belongs
to the owner, the owner's follower count matches, the followers are the next workgroups of the owner's XCD (blockIdx + 8, + 16,
...), no workgroup's range reaches into a third tile (the tile after it would then lack its start), and every packed field fits
its bits (a field that overflowed would break the cover of its neighbour).
The GPU parity tests (tests/test_kernels_gpu.py::test_gemm_nt_stream_k_remainder) run a handful of these configurations; this
sweep covers the rest of the space the dispatch can reach (other models' shapes, reserved-CU grids)."""
import ctypes as C

import pytest


def host_plan(lib, tiles, K, G):
    """(sk_tiles, sk_wgs, P) of an NT product of `tiles` 256 x 256 tiles on G CUs, or None where the plan uses whole tiles."""
    from headct_foundation_amd._lib import HCT_BF16, GemmArgs, GemmPlanInfo
    a = GemmArgs()
    a.M, a.N, a.K = 256 * tiles, 256, K
    a.A, a.a_dtype, a.lda, a.transA = 256, HCT_BF16, K, 0  # (alignment probes: nothing is dereferenced)
    a.B, a.b_dtype, a.ldb, a.transB = 256, HCT_BF16, K, 1
    a.C, a.c_dtype, a.ldc = 256, HCT_BF16, 256
    a.alpha = 1.0
    info = GemmPlanInfo()
    assert lib.hct_gemm_describe(C.byref(a), G, 2 ** 64 - 1, C.byref(info)) == 0
    if not info.sk_tiles:
        return None
    assert info.tiles == tiles and info.grid == G and info.sk_tiles == tiles % G
    return info.sk_tiles, info.sk_wgs, K // 64


def check(lib, G, sk_tiles, sk_wgs, P):
    first, owner = (C.c_uint32 * G)(), (C.c_uint32 * G)()
    assert lib.hct_gemm_stream_k_items(G, sk_tiles, sk_wgs, P, first, owner) == 0
    cover = {}
    for blk in range(G):
        for w in (first[blk], owner[blk]):
            if not w:
                continue
            t, off, n, nf = w & 255, (w >> 8) & 1023, (w >> 18) & 1023, (w >> 28) & 7
            assert (w >> 31) == (off == 0)  # bit 31: the piece starts its tile
            assert 0 <= t < sk_tiles and t < 256 and off < 1024 and 2 <= n <= 1023 and nf <= 7 and off + n <= P
            cover.setdefault(t, []).append((off, n, blk, nf))
    assert sorted(cover) == list(range(sk_tiles))
    for t, pcs in cover.items():
        pcs.sort()
        pos = 0
        for off, n, _, _ in pcs:
            assert off == pos
            pos += n
        assert pos == P
        assert pcs[0][3] == len(pcs) - 1  # the owner (first K range) collects exactly the other pieces ...
        assert [p[2] for p in pcs[1:]] == [pcs[0][2] + 8 * (i + 1) for i in range(len(pcs) - 1)]  # ... from the next workgroups of its XCD


@pytest.mark.parametrize("G", [256, 248, 240, 192, 64, 8])
def test_stream_k_partition_covers_every_remainder_tile_once(lib, G):
    checked = 0
    try:
        lib.hct_debug_set_gemm_variant(-1000 - 512)
        for gain in (1, 8, 20):
            lib.hct_debug_set_gemm_variant(-100 - gain)
            for K in (512, 768, 1024, 1536, 2304, 3072, 4096, 65472):
                for tiles in list(range(1, 2 * G + 2)) + [651, 2604, 1953, 165, 495, 660, 132, 396]:
                    h = host_plan(lib, tiles, K, G)
                    if h is not None:
                        check(lib, G, *h)
                        checked += 1
    finally:
        lib.hct_debug_set_gemm_variant(-100 - 20)
        lib.hct_debug_set_gemm_variant(-1000 - 512)
    if G == 8:  # one workgroup per XCD: nothing to share a tile with
        assert checked == 0
    else:
        assert checked > 100
