"""New texels for a texture on the device (rayhip_scene_set_texture / _device / _blocks; ray_amd/csrc/texture_update.hip.h,
rayhip_textures.hip.h) against the host build of the same element functions (tests/hostsim/hostsim_texture.cpp), which
tests/test_texture_hostsim.py holds against the reference bit for bit.  Pools are read back whole (rayhip_k_read_accel 15, 16) and
compared bitwise; frames are compared bitwise with a fresh upload of the scene the reference built from the new images -- the same
kernels over the same pool bytes."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import texture_cases as T
import util
from ray_amd import hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 64, 64, 4
GPU_TARGETS = ("bc3", "bc4", "bc5_rg", "rgba")  # the three compressed storages and one RGBA texture
GPU_SIZES = ((1, 1), (4, 4), (5, 4), (20, 12), (67, 33))


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert os.path.exists(T.TEX_LIB), "tests/hostsim is not built (run __graft_entry__.build())"
    assert T.have_host_scene_lib(), "oracle/_ref is not built (needs the reference tree at build time)"
    return lib


def _context(lib, blob=None, refit=True):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    if refit:
        ctx.refit_lights(True)  # (before the upload: the upload prepares the tables)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx):
    """RAW, base colour and depth-normals of SPP iterations, as bits"""
    ctx.clear()
    raw = util.render_frames(ctx, SPP).copy()
    return [a.view(np.uint32).copy() for a in (raw, ctx.readback(hip.BUF_BASE_COLOR), ctx.readback(hip.BUF_DEPTH_NORMALS))]


def _same_frames(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def _on_device(texels, offset_bytes=0):
    raw = np.zeros(offset_bytes + texels.nbytes, dtype=np.uint8)
    raw[offset_bytes:] = np.ascontiguousarray(texels).view(np.uint8).ravel()
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset_bytes


def _set(ctx, how, handle, texels):
    if how == "host":
        return ctx.set_texture(handle, texels)
    keep, p = _on_device(texels, 4 if how == "device+4" else 0)
    rc = ctx.set_texture_device(handle, texels.shape[1], texels.shape[0], p)
    del keep  # (the call returned: the device work is done)
    return rc


def _set_and_compare(ctx, how, handles, texels):
    """every texture of `handles` set in turn; after each the whole pool must equal the host build's, only the named texture's words
    may differ from before, and the records stay"""
    for name, handle in handles.items():
        before = T.Pool.of_context(ctx)
        rc, want = T.host_set_texture(before, handle, texels[name])
        assert rc == 0
        assert _set(ctx, how, handle, texels[name]) == 0
        got = T.Pool.of_context(ctx)
        m = before.mask(handle)
        assert np.array_equal(got.words, want.words), (how, name, np.flatnonzero(got.words != want.words)[:8])
        assert np.array_equal(got.words[~m], before.words[~m]) and got.same_meta(before)
        assert not np.array_equal(got.words[m], before.words[m]), (how, name)  # (an update that wrote nothing cannot pass)


# ---- 1: the pool, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", GPU_SIZES, ids=lambda v: str(v))
def test_pool_equals_the_host_build(gpu_lib, w, h):
    images = {t: T.image("random", w, h, 1 + 10 * k) for k, t in enumerate(GPU_TARGETS)}
    blob, handles = T.reference_scene(("gpu", w, h), lambda s: T.pool_scene(s, GPU_TARGETS, images, True))
    assert {t: handles[t] >> 28 for t in GPU_TARGETS} == {"bc3": 5, "bc4": 6, "bc5_rg": 7, "rgba": 0}
    ctx = _context(gpu_lib, blob, refit=False)
    start = T.Pool.of_context(ctx)
    assert np.array_equal(start.words, T.Pool.of_blob(blob).words) and start.same_meta(T.Pool.of_blob(blob)) and start.flags & T.RAW_BC
    for k, how in enumerate(("host", "device", "device+4")):
        new = {t: T.texels_for(t, T.image("gradient" if k == 1 else "random", w, h, 50 + k + 10 * j)) for j, t in enumerate(GPU_TARGETS)}
        _set_and_compare(ctx, how, handles, new)


@pytest.mark.parametrize("odd", [False, True], ids=["eight_bytes_off", "odd_words"])
def test_textures_at_odd_words_and_eight_bytes_off(gpu_lib, odd):
    """The pool packs textures word by word.  A one-block BC4 texture ahead of a BC5 texture puts it 8 bytes off a 16-byte boundary; a
    3 x 3 R8 texture ahead of the block storages puts them at odd words.  Every block texture takes an even number of words, so the
    two cases need a pool each."""
    images = {"bc5_rg": T.image("random", 20, 12, 3), "bc3": T.image("random", 20, 12, 4)}
    blob, handles = T.reference_scene(("alignment", odd), lambda s: T.alignment_scene(s, images, odd))
    pool = T.Pool.of_blob(blob)
    bc5, bc3 = pool.levels(handles["bc5_rg"]), pool.levels(handles["bc3"])
    assert len(bc5) == 3 and len(bc3) == 3
    if odd:
        assert bc3[0][2] % 2 == 1 and bc5[0][2] % 2 == 1, "the block textures do not start at odd words"
    else:
        assert (4 * bc3[0][2]) % 16 == 0 and (4 * bc5[0][2]) % 16 == 8, "the BC5 texture does not start 8 bytes off a 16-byte boundary"
    ctx = _context(gpu_lib, blob, refit=False)
    for k, how in enumerate(("host", "device", "device+4")):
        new = {"bc5_rg": T.texels_for("bc5_rg", T.image("two_colours", 20, 12, 60 + k)), "bc3": T.texels_for("bc3", T.image("grey63", 20, 12, 70 + k))}
        _set_and_compare(ctx, how, handles, new)


@pytest.mark.parametrize("kind", [k for k in T.KINDS if k != "random"])
def test_every_image_kind_at_a_ragged_size(gpu_lib, kind):
    """67 x 33 (153 blocks: more than one workgroup, a ragged tail, four levels): the kinds that take the compressor's other branches"""
    w, h = 67, 33
    images = {t: T.image("random", w, h, 1 + 10 * k) for k, t in enumerate(GPU_TARGETS)}
    blob, handles = T.reference_scene(("gpu", w, h), lambda s: T.pool_scene(s, GPU_TARGETS, images, True))
    ctx = _context(gpu_lib, blob, refit=False)
    _set_and_compare(ctx, "device+4", handles, {t: T.texels_for(t, T.image(kind, w, h, 5 + j)) for j, t in enumerate(GPU_TARGETS)})


# ---- 2: frames ------------------------------------------------------------------------------------------------------------------------
def test_frames_equal_a_fresh_upload(gpu_lib):
    blob_a, (handles, _) = T.reference_scene(("cornell", "A"), lambda s: T.cornell_textures_scene(s, "A"))
    blob_b, (handles_b, _) = T.reference_scene(("cornell", "B"), lambda s: T.cornell_textures_scene(s, "B"))
    assert handles == handles_b and [h >> 28 for h in handles] == [5, 6, 7]
    # (rayhip_clear resets the accumulated image as the reference's Clear does, not the base-colour and depth-normals images, which
    # keep an earlier render's value where a pass writes none: the contexts compared here have rendered equally often)
    frames_a = _frames(_context(gpu_lib, blob_a))
    ctx = _context(gpu_lib, blob_a)
    for handle, texels in zip(handles, T.cornell_texels("B")):
        assert ctx.set_texture(handle, texels) == 0
    got = T.Pool.of_context(ctx)
    assert np.array_equal(got.words, T.Pool.of_blob(blob_b).words) and got.same_meta(T.Pool.of_blob(blob_b))
    frames = _frames(ctx)
    fresh = _frames(_context(gpu_lib, blob_b))
    assert _same_frames(frames, fresh)
    assert not any(np.array_equal(a, b) for a, b in zip(frames[:2], frames_a[:2]))  # RAW and base colour differ from set A's
    assert not _same_frames(frames, frames_a)


# ---- 3: ready blocks --------------------------------------------------------------------------------------------------------------------
def test_ready_blocks_for_a_bc1_texture(gpu_lib):
    blob_a, handles = T.reference_scene(("blocks", "A"), lambda s: T.cornell_block_scene(s, T.BLOCK_SEEDS))
    seeds = dict(T.BLOCK_SEEDS, bc1=41)
    blob_b, _ = T.reference_scene(("blocks", "bc1"), lambda s: T.cornell_block_scene(s, seeds))
    frames_a = _frames(_context(gpu_lib, blob_a))  # (a context of its own: see test_frames_equal_a_fresh_upload)
    ctx = _context(gpu_lib, blob_a)
    assert handles["bc1"] >> 28 == 4
    assert ctx.set_texture_blocks(handles["bc1"], T.block_data("bc1", 41)) == 0
    got, want = T.Pool.of_context(ctx), T.Pool.of_blob(blob_b)
    assert np.array_equal(got.words, want.words) and got.same_meta(want)
    frames = _frames(ctx)
    assert _same_frames(frames, _frames(_context(gpu_lib, blob_b))) and not _same_frames(frames, frames_a)


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_touches_nothing(gpu_lib, monkeypatch):
    import env_cases as E

    err = lambda: gpu_lib.fn("last_error")().decode()  # noqa: E731
    images = {t: T.image("random", 20, 12, 1 + 10 * k) for k, t in enumerate(GPU_TARGETS)}
    blob, handles = T.reference_scene(("gpu", 20, 12), lambda s: T.pool_scene(s, GPU_TARGETS, images, True))
    ctx = _context(gpu_lib, blob, refit=False)
    before = T.Pool.of_context(ctx)
    t = T.texels_for("bc3", T.image("random", 20, 12, 99))
    keep, p = _on_device(t)
    fn = gpu_lib.fn
    untouched = lambda c, held: np.array_equal(T.Pool.of_context(c).words, held.words) and T.Pool.of_context(c).same_meta(held)  # noqa: E731
    # 1: null pointers, handles outside the tables, sizes, alignment
    for call in (lambda: fn("scene_set_texture")(ctx._ctx, handles["bc3"], 20, 12, None), lambda: fn("scene_set_texture_device")(ctx._ctx, handles["bc3"], 20, 12, None),
                 lambda: fn("scene_set_texture_blocks")(ctx._ctx, handles["bc3"], None, 240)):
        assert call() == 1 and "null pointer" in err()
    for call, match in ((lambda: ctx.set_texture(0x80000000, t), "names no texture"), (lambda: ctx.set_texture(0xffffffff, t), "names no texture"),
                        (lambda: ctx.set_texture((5 << 28) | T.YCOCG_BIT | 3, t), "names no texture"), (lambda: ctx.set_texture((7 << 28) | 3, t), "names no texture"),
                        (lambda: ctx.set_texture(handles["bc3"], t[:, :-1]), "19 x 12"), (lambda: ctx.set_texture(handles["rgba"], t.T.copy()), "12 x 20"),
                        (lambda: ctx.set_texture_device(handles["bc4"], 12, 20, p), "12 x 20"), (lambda: ctx.set_texture_device(handles["bc3"], 20, 12, p + 2), "4-byte aligned"),
                        (lambda: ctx.set_texture_blocks(handles["bc3"], np.zeros(8, np.uint8)), "8 bytes"),
                        (lambda: ctx.set_texture_blocks(handles["rgba"], np.zeros(20 * 12 * 4, np.uint8)), "not blocks")):
        with pytest.raises(RuntimeError, match=match):
            call()
        assert untouched(ctx, before), match
    # 2: a storage-5 texture named without its YCoCg bit has no compressor
    assert ctx.set_texture(handles["bc3"] & ~T.YCOCG_BIT, t) == 2 and "BC1 or plain BC3" in err() and untouched(ctx, before)
    # 2: no scene
    none = hip.Context(0, gpu_lib)
    assert none.set_texture(handles["bc3"], t) == 2 and err() and none.set_texture_device(handles["bc3"], 20, 12, p) == 2 and err()
    assert none.set_texture_blocks(handles["bc3"], np.zeros(240, np.uint8)) == 2 and err()
    # 2: BC1 and plain BC3 given to the texel forms
    blob_k, block_handles = T.reference_scene(("blocks", "A"), lambda s: T.cornell_block_scene(s, T.BLOCK_SEEDS))
    bctx = _context(gpu_lib, blob_k, refit=False)
    held = T.Pool.of_context(bctx)
    for name in ("bc1", "bc3"):
        w, h = T.BLOCK_TEXTURES[name][1:3]
        assert bctx.set_texture(block_handles[name], np.zeros((h, w), np.uint32)) == 2 and "ready blocks" in err() and untouched(bctx, held)
    # 2: a block storage on a scene uploaded decoded
    monkeypatch.setenv("RAY_HIP_DECODE_BC", "1")
    blob_d, handles_d = T.reference_scene(("gpu", 20, 12, "decoded"), lambda s: T.pool_scene(s, GPU_TARGETS, images, True))
    monkeypatch.delenv("RAY_HIP_DECODE_BC")
    dctx = _context(gpu_lib, blob_d, refit=False)
    held = T.Pool.of_context(dctx)
    assert not held.flags & T.RAW_BC and handles_d == handles
    assert dctx.set_texture(handles["bc3"], t) == 2 and "decoded" in err() and dctx.set_texture_device(handles["bc4"], 20, 12, p) == 2 and "decoded" in err()
    assert dctx.set_texture_blocks(handles["bc3"], np.zeros(240, np.uint8)) == 2 and "decoded" in err() and untouched(dctx, held)
    assert dctx.set_texture(handles["rgba"], t) == 0  # (its uncompressed textures still take texels)
    # 1: the environment map has its own call
    eblob = E.map_blob("16x8")
    ectx = _context(gpu_lib, eblob)
    held = T.Pool.of_context(ectx)
    env_map = int(E.blob_env(eblob)["env_map"])
    with pytest.raises(RuntimeError, match="environment map"):
        ectx.set_texture(env_map, np.zeros((8, 16), np.uint32))
    with pytest.raises(RuntimeError, match="environment map"):
        ectx.set_texture(env_map & 0xf0ffffff, np.zeros((8, 16), np.uint32))  # (the handle's flags do not name another texture)
    assert untouched(ectx, held)
    del keep
    assert untouched(ctx, before)


# ---- 5: order with the other calls ------------------------------------------------------------------------------------------------------
def test_it_commutes_with_set_materials_and_survives_moved_instances(gpu_lib):
    blob_a, (handles, _) = T.reference_scene(("cornell", "A"), lambda s: T.cornell_textures_scene(s, "A"))
    texels = T.cornell_texels("B")
    one, other = _context(gpu_lib, blob_a), _context(gpu_lib, blob_a)
    mats = one.read_accel(11).copy()
    red = int(np.flatnonzero((mats["base_color"] == np.array([0.5, 0.0, 0.0], np.float32)).all(axis=1))[0])
    record = mats[red:red + 1].copy()
    record["base_color"][0] = (0.1, 0.2, 0.7)
    slots = np.array([red], dtype=np.uint32)
    for handle, t in zip(handles, texels):
        assert one.set_texture(handle, t) == 0
    assert one.set_materials(slots, record) == 0
    assert other.set_materials(slots, record) == 0
    for handle, t in zip(handles, texels):
        assert other.set_texture(handle, t) == 0
    state = lambda c: (T.Pool.of_context(c).words, c.read_accel(16).copy(), c.read_accel(11).copy().view(np.uint32))  # noqa: E731
    assert all(np.array_equal(a, b) for a, b in zip(state(one), state(other)))
    assert not np.array_equal(state(one)[0], T.Pool.of_blob(blob_a).words)
    assert _same_frames(_frames(one), _frames(other))
    # moved instances: the texels stay
    held = T.Pool.of_context(one)
    xform = one.read_accel(8)["xform"][:1].astype(np.float32).reshape(1, 16).copy()
    xform[0, 12] += np.float32(0.01)
    assert one.set_instance_transforms(np.array([0], dtype=np.uint32), xform) == 0
    after = T.Pool.of_context(one)
    assert np.array_equal(after.words, held.words) and after.same_meta(held)
    # ... and the texture still takes new texels behind them
    back = T.cornell_texels("A")
    assert one.set_texture(handles[0], back[0]) == 0
    rc, want = T.host_set_texture(held, handles[0], back[0])
    assert rc == 0 and np.array_equal(T.Pool.of_context(one).words, want.words)
