"""New texels for a texture of the pool, host build against the reference (no GPU).

tests/hostsim/hostsim_texture.cpp compiles ray_amd/csrc/texture_update.h -- the block emitters of the BC3-YCoCg, BC4 and BC5 storages,
the clamped gather of incomplete blocks, the mip average -- as plain loops.  The reference's host code (its AddTexture, its real-time
block compressor in the _SSE2 forms this x86 build runs, its mip builder) builds every scene twice, from image set A and from set B;
hostsim_set_texture of B's texels on A's pool must give B's pool BIT FOR BIT, with every other texture's words unchanged.

Sizes (generate_mipmaps on unless said): 1 x 1 one level, one incomplete block; 3 x 5 one level, incomplete blocks; 4 x 4 levels 4 and 2,
the last one an incomplete block; 5 x 4 an incomplete column, levels 5 x 4 and 2 x 2; 16 x 16 levels 16, 8, 4, 2; 20 x 12 levels
20 x 12, 10 x 6, 5 x 3; 67 x 33 a ragged grid of 17 x 9 blocks; 64 x 32; 16 x 16 without mips.

No block was found on which the reference's _Ref and _SSE2 forms could disagree (DESIGN.md section 10 says why they cannot on the
ranges that occur), so there is no named case of that kind; test_the_scale_branches_are_taken names the blocks that take each branch
of ScaleYCoCg instead."""
import os

import numpy as np
import pytest

import texture_cases as T

pytestmark = pytest.mark.skipif(not T.have_host_scene_lib(), reason="oracle/_ref is not built (needs the reference tree at build time)")


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(T.TEX_LIB), "tests/hostsim is not built (run __graft_entry__.build())"


def _images(kind, w, h, seed):
    return {t: T.image(kind, w, h, seed + 10 * k) for k, t in enumerate(T.TARGETS)}


def _pair(key, targets, w, h, mips, kind, compress=True, odd=True):
    out = []
    for seed in (1, 2):
        images = {t: T.image(kind, w, h, seed + 10 * k) for k, t in enumerate(targets)}
        blob, handles = T.reference_scene((key, targets, w, h, mips, kind, compress, odd, seed),
                                          lambda s, images=images: T.pool_scene(s, targets, images, mips, odd), compress)
        out.append((T.Pool.of_blob(blob), handles, images))
    return out


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("w,h,mips", T.SIZES, ids=lambda v: str(v))
def test_pool_equals_the_references(w, h, mips, kind):
    (a, handles, _), (b, handles_b, images_b) = _pair("pool", T.TARGETS, w, h, mips, kind)
    assert a.flags & T.RAW_BC and a.same_meta(b)
    storages = {t: handles[t] >> 28 for t in T.TARGETS}
    assert storages == {"bc3": 5, "bc4": 6, "bc5_rgba": 7, "bc5_rg": 7} and handles["bc3"] & T.YCOCG_BIT
    assert {t: handles[t] & 0xf0ffffff for t in T.TARGETS} == {t: handles_b[t] & 0xf0ffffff for t in T.TARGETS}  # (B's blue may flip reconstruct_z)
    expected_levels = 1
    while mips and min(w >> (expected_levels - 1), h >> (expected_levels - 1)) >= 4:
        expected_levels += 1
    pool = a
    for t in T.TARGETS:
        assert len(a.levels(handles[t])) == expected_levels
        rc, after = T.host_set_texture(pool, handles[t], T.texels_for(t, images_b[t]))
        assert rc == 0
        m = a.mask(handles[t])
        assert np.array_equal(after.words[m], b.words[m]), (t, np.flatnonzero(after.words[m] != b.words[m])[:8])
        assert np.array_equal(after.words[~m], pool.words[~m]) and after.same_meta(a)
        pool = after
    assert np.array_equal(pool.words, b.words)  # every target changed, every neighbour as it was: B's pool


def test_pool_equals_the_references_at_even_words():
    """the same pool without the 3 x 3 texture: block textures on even words"""
    (a, handles, _), (b, _, images_b) = _pair("even", T.TARGETS, 20, 12, True, "random", odd=False)
    pool = a
    for t in T.TARGETS:
        rc, pool = T.host_set_texture(pool, handles[t], T.texels_for(t, images_b[t]))
        assert rc == 0
    assert np.array_equal(pool.words, b.words) and not np.array_equal(a.words, b.words)


def test_the_scale_branches_are_taken():
    """storage 5: near-grey blocks whose chroma stays within 31 / 63 of 128 carry scale 4 / 2 (byte 2 of both end points: 24 / 8 -> the
    blue five bits 3 / 1), random bytes scale 1 -- ScaleYCoCg's three outcomes, named"""
    for kind, blue in (("grey31", 3), ("grey63", 1), ("alternating", 3)):
        block = T.host_block(5, T.words_of(T.image(kind, 4, 4, 1)))
        assert (int(block[2]) & 31, (int(block[2]) >> 16) & 31) == (blue, blue), kind
    wide = T.image("random", 4, 4, 1)
    wide[0, 0, :3], wide[0, 1, :3] = (255, 0, 0), (0, 0, 255)  # Co at both ends
    block = T.host_block(5, T.words_of(wide))
    assert (int(block[2]) & 31, (int(block[2]) >> 16) & 31) == (0, 0)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (20, 12)])
def test_uncompressed_storages_take_the_words(w, h):
    (a, handles, _), (b, _, images_b) = _pair("plain", T.PLAIN, w, h, True, "random", compress=False)
    assert {t: handles[t] >> 28 for t in T.PLAIN} == {"rgba": 0, "rgb": 1, "rg": 2, "r": 3}
    pool = a
    for t in T.PLAIN:
        assert len(a.levels(handles[t])) == 1  # (the swizzled storage builds no mips)
        rc, pool = T.host_set_texture(pool, handles[t], T.texels_for(t, images_b[t]))
        assert rc == 0
    assert np.array_equal(pool.words, b.words) and not np.array_equal(a.words, b.words)


def test_ready_blocks_equal_the_export():
    """BC1 and plain BC3 (and BC4, BC5) take ready blocks for their whole chain: the pool equals the export of a scene built from them"""
    blob_a, handles = T.reference_scene(("blocks", "A"), lambda s: T.cornell_block_scene(s, T.BLOCK_SEEDS))
    a = T.Pool.of_blob(blob_a)
    assert {n: handles[n] >> 28 for n in handles} == {"bc1": 4, "bc3": 5, "bc4": 6, "bc5": 7} and not handles["bc3"] & T.YCOCG_BIT
    for name in ("bc1", "bc3", "bc4", "bc5"):
        seeds = dict(T.BLOCK_SEEDS, **{name: 40 + T.BLOCK_SEEDS[name]})
        blob_b, _ = T.reference_scene(("blocks", name), lambda s, seeds=seeds: T.cornell_block_scene(s, seeds))
        b = T.Pool.of_blob(blob_b)
        data = T.block_data(name, seeds[name])
        rc, after = T.host_set_texture_blocks(a, handles[name], data)
        assert rc == 0 and a.same_meta(b)
        assert np.array_equal(after.words, b.words) and not np.array_equal(a.words, b.words)
        assert T.host_set_texture_blocks(a, handles[name], data[:-8])[0] == 1
        # the texel forms have no compressor for BC1 and plain BC3
        w, h = T.BLOCK_TEXTURES[name][1:3]
        rc, same = T.host_set_texture(a, handles[name], np.zeros((h, w), np.uint32))
        assert rc == (2 if name in ("bc1", "bc3") else 0) and (rc == 0 or np.array_equal(same.words, a.words))


def test_refusals_of_the_host_build():
    (a, handles, images), _ = _pair("pool", T.TARGETS, 20, 12, True, "random")
    t = T.texels_for("bc3", images["bc3"])
    for handle, texels, code in ((handles["bc3"], t[:, :-1], 1), (handles["bc3"], t.T, 1), (0x80000000, t, 1), ((5 << 28) | 99, t, 1), (handles["bc3"] & ~T.YCOCG_BIT, t, 2)):
        rc, after = T.host_set_texture(a, handle, texels)
        assert rc == code and np.array_equal(after.words, a.words)
    decoded = a.copy()
    decoded.flags = 0
    assert T.host_set_texture(decoded, handles["bc4"], t)[0] == 2
