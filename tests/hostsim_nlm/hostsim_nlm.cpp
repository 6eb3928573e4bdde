// hostsim_nlm.cpp -- TEST INFRASTRUCTURE.  The host build of tests/hostsim/hostsim.cpp, whole and unchanged, with its variance image
// in reach: hostsim_denoise_nlm reads the variance estimate from the context's `temp` buffer, which the plain host build can neither
// import nor show.  This library is that source plus
//   * bit 3 (RAYHIP_REDUCE_VARIANCE) of an explicit mask in hostsim_owned_bytes / _export_owned / _import_owned: `temp`, behind the
//     images the lower bits select, as rayhip_import_owned lays them out (`what` == 0 keeps meaning the first three images);
//   * RAYHIP_BUF_VARIANCE in hostsim_readback: `temp`.
// The four entry points of the plain source are compiled under other names and called for everything else, so whatever
// tests/hostsim/_build/libhostsim.so computes this library computes too (tests/test_nlm_model_hostsim.py holds it to that).
//
// Why a library of its own and not ten lines in hostsim.cpp: tests/hostsim/ and the libraries built from it are the checker of every
// other host-build test, and the suite of the commit before this one has to run on the build of this one.  With tests/hostsim/ left
// byte for byte as it was, that holds by construction; the NLM tests alone depend on what is added here.
#define hostsim_readback hostsim_plain_readback
#define hostsim_owned_bytes hostsim_plain_owned_bytes
#define hostsim_export_owned hostsim_plain_export_owned
#define hostsim_import_owned hostsim_plain_import_owned
#include "../hostsim/hostsim.cpp"
#undef hostsim_readback
#undef hostsim_owned_bytes
#undef hostsim_export_owned
#undef hostsim_import_owned

namespace {
// the mask the plain entry points see (0: none of their images is selected) and whether the variance image is selected
uint32_t plain_mask(const uint32_t what) { return what == 0 ? 7u : (what & 7u); }
bool with_variance(const uint32_t what) { return (what & uint32_t(RAYHIP_REDUCE_VARIANCE)) != 0; }
int plain_images(const uint32_t what) { return __builtin_popcount(plain_mask(what)); }
// float4 slots of one image in the packed buffer of rank `rank` of `nranks`
size_t image_slots(const hostsim_ctx *c, const int nranks, const int rank) {
    const ShardTiles st = shard_tiles(c->w, c->h, c->shard.tile);
    return size_t(shard_owned_tiles(st.total, nranks, rank)) * size_t(c->shard.tile) * size_t(c->shard.tile);
}
} // namespace

HS_API int hostsim_readback(hostsim_ctx *c, int which, float *dst, int pitch_px) {
    if (which != RAYHIP_BUF_VARIANCE) {
        return hostsim_plain_readback(c, which, dst, pitch_px);
    }
    for (int y = 0; y < c->h; ++y) {
        memcpy(dst + size_t(y) * pitch_px * 4, c->temp.data() + size_t(y) * c->w, size_t(c->w) * 16);
    }
    return 0;
}

HS_API size_t hostsim_owned_bytes(hostsim_ctx *c, uint32_t what, int nranks, int rank) {
    return image_slots(c, nranks, rank) * 16u * size_t(plain_images(what) + (with_variance(what) ? 1 : 0));
}

HS_API int hostsim_export_owned(hostsim_ctx *c, uint32_t what, void *dst, size_t capacity) {
    if (hostsim_owned_bytes(c, what, c->shard.count, c->shard.index) > capacity) {
        g_err = "hostsim_export_owned: destination too small";
        return 1;
    }
    if (plain_mask(what) != 0 && hostsim_plain_export_owned(c, plain_mask(what), dst, capacity)) {
        return 1;
    }
    if (with_variance(what)) {
        const size_t n = image_slots(c, c->shard.count, c->shard.index);
        float4 *out = static_cast<float4 *>(dst) + size_t(plain_images(what)) * n;
        for (size_t i = 0; i < n; ++i) {
            int x, y;
            out[i] = shard_slot_pixel(c->shard, c->w, c->h, int(i), x, y) ? c->temp[size_t(y) * c->w + x] : float4{0, 0, 0, 0};
        }
    }
    return 0;
}

HS_API int hostsim_import_owned(hostsim_ctx *c, uint32_t what, int from_rank, const void *src, size_t bytes) {
    if (from_rank < 0 || from_rank >= c->shard.count || bytes < hostsim_owned_bytes(c, what, c->shard.count, from_rank)) {
        g_err = "hostsim_import_owned: bad rank or short buffer";
        return 1;
    }
    if (plain_mask(what) != 0 && hostsim_plain_import_owned(c, plain_mask(what), from_rank, src, bytes)) {
        return 1;
    }
    if (with_variance(what) && from_rank != c->shard.index) {
        const Shard sender = {c->shard.tile, c->shard.count, from_rank};
        const size_t n = image_slots(c, c->shard.count, from_rank);
        const float4 *in = static_cast<const float4 *>(src) + size_t(plain_images(what)) * n;
        for (size_t i = 0; i < n; ++i) {
            int x, y;
            if (shard_slot_pixel(sender, c->w, c->h, int(i), x, y)) {
                c->temp[size_t(y) * c->w + x] = in[i];
            }
        }
    }
    return 0;
}
