// hostsim_morph.cpp -- TEST INFRASTRUCTURE.  Morph targets as the device applies them (ray_amd/csrc/morph.h: the row table of a set's
// targets, the posed record of a vertex, alone and ahead of a skin), compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma
// contraction, SSE2, glibc libm) over plain arrays, with the prefix hostsim_ and without a context.  tests/test_morph_hostsim.py holds
// these against a numpy restatement; tests/test_gpu_morph.py holds the device (morph.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/morph.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// what rayhip_morph_create says of a description's targets: 0 = fine, 1 = null pointer / targets_count outside 1..65536 / indices not
// strictly ascending or >= count / a delta that is not finite / too many entries (morph.h: validate_targets tells them apart in *why)
HS_API int hostsim_morph_validate(const rayhip_morph_target *targets, uint32_t targets_count, uint32_t count, int *why) {
    *why = 0;
    if (!targets || targets_count == 0 || targets_count > rayhip_morph::MAX_TARGETS) {
        *why = targets ? 5 : 1;
        return 1;
    }
    uint32_t where = 0;
    *why = rayhip_morph::validate_targets(targets, targets_count, count, where);
    return *why ? 1 : 0;
}

// the row table of (valid) targets: row[count + 1]; entries[entries_room] records of 40 bytes (target, dp, dn, db).  Returns the number
// of entries; nothing is written into `entries` where it exceeds the room (call again with more).
HS_API uint32_t hostsim_morph_rows(const rayhip_morph_target *targets, uint32_t targets_count, uint32_t count, uint32_t *row, void *entries,
                                   uint32_t entries_room) {
    std::vector<uint32_t> r;
    std::vector<rayhip_morph::Entry> e;
    rayhip_morph::build_rows(targets, targets_count, count, r, e);
    memcpy(row, r.data(), r.size() * sizeof(uint32_t));
    if (e.size() <= entries_room && !e.empty()) {
        memcpy(entries, e.data(), e.size() * sizeof(rayhip_morph::Entry));
    }
    return uint32_t(e.size());
}

// out[count]: base[count] posed by weights[targets_count] over the row table; `used`: per vertex, or null (all in use).  Returns the
// number of vertices in use whose posed position is not finite.
HS_API uint32_t hostsim_morph_vertices(const rayhip_vertex *base, const uint32_t *row, const void *entries, uint32_t count, const float *weights,
                                       const uint8_t *used, rayhip_vertex *out) {
    return rayhip_morph::morph_vertices_host(base, row, static_cast<const rayhip_morph::Entry *>(entries), count, weights, used, out);
}

// ... and ahead of a skin (indices / skin_weights [count][4], bones [..][12]): the composition
HS_API uint32_t hostsim_morph_skin_vertices(const rayhip_vertex *base, const uint32_t *row, const void *entries, uint32_t count, const float *weights,
                                            const uint16_t *indices, const float *skin_weights, const float *bones, const uint8_t *used, rayhip_vertex *out) {
    return rayhip_morph::morph_skin_vertices_host(base, row, static_cast<const rayhip_morph::Entry *>(entries), count, weights, indices, skin_weights, bones,
                                                  used, out);
}

// weight arrays up to this many targets are read from LDS by the device kernels, longer ones from memory
HS_API uint32_t hostsim_morph_lds_targets(void) { return rayhip_morph::MORPH_LDS_TARGETS; }
