"""CPU: the tile walk of the persistent NT GEMM (csrc/gemm_plan.h: nt_walk_width on the host, nt_walk_id inside dp_id of
gemm_bf16_nt256_kernel), queried from the library itself (hct_gemm_describe, hct_gemm_nt_walk: host arithmetic, no device call).

* virtual block id -> tile id (nt_xcd_pos, then nt_walk_id) is a bijection onto the whole tiles [sk_tiles, tiles) for every band
  width, for tile counts that are no multiple of 8 (the XCDs' slices then differ in length: 7 x 3, 55 x 5, 217 x 9, ...) and with
  or without a stream-K remainder in front;
* inside a band the column tile runs fastest and the row tile never goes back, so that 32 consecutive positions (one XCD's round)
  hold at most `width` weight panels and consecutive rounds of a slice keep them;
* the width nt_walk_width chooses (hook -20 - 79; the default plan uses no bands) keeps the window's weight panels inside their share of an XCD's L2 (half of 4 MiB) for the
  multi-round shapes of ViT-B, ViT-L and the DINO head, and leaves single-round launches and long-K panels alone."""
import ctypes as C

import pytest

L2_BYTES = 4 << 20
WEIGHT_BUDGET = L2_BYTES // 2


def walk_vb(lib, tiles, ntn, sk, w):
    """tile id of every virtual block id vb (XCD = vb & 7)"""
    ids = (C.c_int * max(1, tiles - sk))()
    assert lib.hct_gemm_nt_walk(tiles, ntn, sk, w, ids) == 0
    return list(ids)[:tiles - sk]


def walk(lib, tiles, ntn, sk, w):
    """tile ids in walk order: the eight XCDs' slices one after the other (the first nwg % 8 of them one longer)"""
    by_vb = walk_vb(lib, tiles, ntn, sk, w)
    return [i for x in range(8) for i in by_vb[x::8]]


@pytest.mark.parametrize("ntn", [1, 2, 3, 5, 9, 12, 16])
def test_walk_is_a_bijection_onto_the_whole_tiles(lib, ntn):
    for ntm in (1, 2, 3, 7, 55, 217):
        tiles = ntm * ntn
        for sk in sorted({0, 1, ntn - 1, ntn, ntn + 1, min(tiles, 139), tiles % 256 if tiles > 256 else 0}):
            if sk > tiles or sk >= 256:
                continue
            for w in list(range(0, ntn + 2)) + [79]:
                ids = walk(lib, tiles, ntn, sk, w)
                assert sorted(walk_vb(lib, tiles, ntn, sk, w)) == list(range(sk, tiles)), (ntm, ntn, sk, w)
                if w <= 0 or w >= ntn:
                    assert ids == list(range(sk, tiles))  # no bands: n fastest over all of N


@pytest.mark.parametrize("ntm,ntn,sk,w", [(217, 12, 0, 4), (217, 9, 0, 5), (217, 12, 44, 4), (55, 12, 0, 6), (100, 16, 17, 4), (31, 7, 3, 2)])
def test_walk_keeps_a_band_while_it_goes_down_m(lib, ntm, ntn, sk, w):
    tiles = ntm * ntn
    ids = walk(lib, tiles, ntn, sk, w)
    r0 = -(-sk // ntn)
    lead = min(r0 * ntn, tiles) - sk
    assert ids[:lead] == list(range(sk, sk + lead))  # the rest of the row the stream-K remainder ends in
    body = ids[lead:]
    rows = ntm - r0
    pos = 0
    for b in range(-(-ntn // w)):
        wb = min(w, ntn - b * w)
        band = body[pos:pos + rows * wb]
        pos += rows * wb
        assert [i % ntn for i in band] == [b * w + j for _ in range(rows) for j in range(wb)]
        assert [i // ntn for i in band] == [r0 + r for r in range(rows) for _ in range(wb)]
        for s in range(0, len(band), 32):  # any aligned window of 32 positions: at most w weight panels
            assert len({i % ntn for i in band[s:s + 32]}) <= w
    assert pos == len(body)


def plan(lib, M, N, K, G=256):
    from headct_foundation_amd._lib import HCT_BF16, GemmArgs, GemmPlanInfo
    a = GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.A, a.a_dtype, a.lda, a.transA = 256, HCT_BF16, K, 0  # (alignment probes: nothing is dereferenced)
    a.B, a.b_dtype, a.ldb, a.transB = 256, HCT_BF16, K, 1
    a.C, a.c_dtype, a.ldc = 256, HCT_BF16, N
    a.alpha = 1.0
    info = GemmPlanInfo()
    assert lib.hct_gemm_describe(C.byref(a), G, 2 ** 64 - 1, C.byref(info)) == 0
    return info


@pytest.fixture
def bands(lib):
    """plans with nt_walk_width's bands instead of the default (none)"""
    lib.hct_debug_set_gemm_variant(-20 - 79)
    yield
    lib.hct_debug_set_gemm_variant(-20)


# (M, N, K): decoder and encoder products of the MAE step at batch 256 (ViT-B: 217 / 55 tokens per volume; ViT-L: width 1024), the
# DINO projection head's last Linear, and the multi-round shapes of a data-parallel grid that leaves 16 CUs free
VITB = [(55552, 3072, 768), (55552, 2304, 768), (55552, 768, 768), (55552, 768, 3072), (14080, 3072, 768), (14080, 2304, 768),
        (14080, 768, 768), (14080, 768, 3072)]
VITL = [(55552, 4096, 1024), (55552, 3072, 1024), (55552, 1024, 1024), (55552, 1024, 4096), (14080, 4096, 1024)]
DINO = [(2560, 65536, 256), (512, 65536, 256), (2560, 2048, 768), (2560, 256, 2048)]


@pytest.mark.parametrize("M,N,K", VITB + VITL + DINO)
@pytest.mark.parametrize("G", [256, 240])
def test_chosen_width_respects_the_l2_budget(lib, bands, M, N, K, G):
    info = plan(lib, M, N, K, G)
    assert info.kernel == 2  # HCT_GEMM_NT256
    ntn = -(-N // 256)
    w = info.walk_width
    assert 1 <= w <= ntn
    panel = 256 * K * 2
    if w < ntn:  # banded: more than one round, at least two panels per band, inside the budget, and no wider band would fit it
        assert info.tiles > G
        assert 2 <= w and w * panel <= WEIGHT_BUDGET
        bands = -(-ntn // w)
        assert w == -(-ntn // bands)  # bands of (nearly) equal width
        assert bands == 1 or -(-ntn // (bands - 1)) * panel > WEIGHT_BUDGET  # ... and no fewer bands would do
    else:        # one band: a single round, or the row already fits, or panels too long for two of them to fit
        assert info.tiles <= G or ntn * panel <= WEIGHT_BUDGET or 2 * panel > WEIGHT_BUDGET
    ids = walk(lib, info.tiles, ntn, info.sk_tiles, w)
    assert sorted(ids) == list(range(info.sk_tiles, info.tiles))


def test_default_plan_has_no_bands(lib):
    for M, N, K in VITB + VITL + DINO:
        assert plan(lib, M, N, K).walk_width == -(-N // 256)


def test_flagship_shapes_get_the_expected_widths(lib, bands):
    assert plan(lib, 55552, 3072, 768).walk_width == 4    # 12 column tiles: 3 bands of 4 (4 x 384 KiB = 1.5 MiB of weights)
    assert plan(lib, 55552, 2304, 768).walk_width == 5    # 9 column tiles: bands of 5 and 4
    assert plan(lib, 55552, 768, 768).walk_width == 3     # the whole row: 3 panels fit
    assert plan(lib, 55552, 768, 3072).walk_width == 3    # 1.5-MiB panels: no bands
    assert plan(lib, 14080, 768, 768).walk_width == 3     # a single round of 192-row tiles


def test_forced_width_hook(lib):
    try:
        lib.hct_debug_set_gemm_variant(-20 - 6)
        assert plan(lib, 55552, 3072, 768).walk_width == 6 and plan(lib, 55552, 768, 768).walk_width == 3
        lib.hct_debug_set_gemm_variant(-20 - 79)
        assert plan(lib, 55552, 3072, 768).walk_width == 4
    finally:
        lib.hct_debug_set_gemm_variant(-20)
    assert plan(lib, 55552, 3072, 768).walk_width == 12
