// morph.h -- morph targets (blend shapes) of the vertices a morph set drives (rayhip_morph_create / rayhip_scene_pose): the base
// records and the targets' deltas stay on the device, a pose is one weight per target.  Element functions shared by the device
// kernels (morph.hip.h) and a plain-loop host driver (tests/hostsim/hostsim_morph.cpp), like skin.h: IEEE operations in a STATED
// ORDER without contraction on both sides, so both produce the same bits.
//
// Targets are SPARSE: the caller names, per target, the vertices it moves.  rayhip_morph_create turns the lists into a per-vertex row
// table, a gather form (build_rows: a counting sort): row[count + 1] offsets into one entry array sorted by vertex and, within a
// vertex, by ascending target number.  No atomics, and a vertex's sum has a fixed order.
// The posed record of a vertex, from its base record and the entries of its row in order:
//   p, n, b start as base.p, base.n, base.b
//   per entry of target t:  w = weights[t]; skipped where w == 0; else p_i = p_i + w * dp_i, n_i = n_i + w * dn_i, b_i = b_i + w * db_i
//              (i = 0..2: one multiply, then one add)
//   no entry used: the base record bytewise.  Otherwise position p; normal and bitangent normalised as skin.h normalises
//              (normalised_or_rest, the fallback being the BASE vector); uv copied.
// Any finite weight is allowed (negative ones and ones above 1 are in use).
//
// MORPH, THEN SKIN: for a vertex that lies in a morph set and in a skin the posed record is skin_vertex(morph_vertex(base ...),
// influences, palette) -- the skin's own rest record is not read, and the fallback of the skin's normalisation is the morphed vector.
#pragma once

#include <stdint.h>

#include <vector>

#include "rt_types.h"
#include "skin.h"

namespace rayhip_morph {

constexpr uint32_t MAX_MORPHS = 16;           // live morph sets per context
constexpr uint32_t MAX_TARGETS = 65536;       // targets per set
constexpr uint32_t MORPH_LDS_TARGETS = 1024;  // weight arrays up to this length are copied to LDS by the block (4 KB)

// one entry of a vertex's row: what target `target` adds to the vertex at weight 1 (40 bytes)
struct Entry {
    uint32_t target;
    float dp[3], dn[3], db[3];
};
static_assert(sizeof(Entry) == 40, "rows are read as 40-byte records");

// the running sums of one vertex: morph_begin, morph_add over the entries of its row in order (in one piece or several), morph_end
struct Sums {
    float p[3], n[3], b[3];
    bool used;
};

RT_HD void morph_begin(const rayhip_vertex &base, Sums &s) {
    for (int i = 0; i < 3; ++i) {
        s.p[i] = base.p[i], s.n[i] = base.n[i], s.b[i] = base.b[i];
    }
    s.used = false;
}

RT_HD void morph_add(const Entry *entries, const uint32_t n, const float *weights, Sums &s) {
    for (uint32_t k = 0; k < n; ++k) {
        const Entry &e = entries[k];
        const float w = weights[e.target];
        if (w == 0.0f) {
            continue;
        }
        for (int i = 0; i < 3; ++i) {
            s.p[i] = s.p[i] + w * e.dp[i];
            s.n[i] = s.n[i] + w * e.dn[i];
            s.b[i] = s.b[i] + w * e.db[i];
        }
        s.used = true;
    }
}

RT_HD void morph_end(const rayhip_vertex &base, const Sums &s, rayhip_vertex &out) {
    out = base;
    if (!s.used) {
        return; // (no entry, or none with a weight: the base record)
    }
    out.p[0] = s.p[0], out.p[1] = s.p[1], out.p[2] = s.p[2];
    rayhip_skin::normalised_or_rest(s.n, base.n, out.n);
    rayhip_skin::normalised_or_rest(s.b, base.b, out.b);
}

// the posed record of one vertex: `entries` are the `n` of its row.  Their targets are below the weight count (build_rows made them).
RT_HD void morph_vertex(const rayhip_vertex &base, const Entry *entries, const uint32_t n, const float *weights, rayhip_vertex &out) {
    Sums s;
    morph_begin(base, s);
    morph_add(entries, n, weights, s);
    morph_end(base, s, out);
}

// ... and of a vertex that a skin covers too: the composition, literally
RT_HD void morph_skin_vertex(const rayhip_vertex &base, const Entry *entries, const uint32_t n, const float *weights, const uint16_t idx[4], const float w[4],
                             const float *bones, rayhip_vertex &out) {
    rayhip_vertex morphed;
    morph_vertex(base, entries, n, weights, morphed);
    rayhip_skin::skin_vertex(morphed, idx, w, bones, out);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// what rayhip_morph_create checks of a description's targets (the pointers of the description itself are the caller's to check):
// 0 = fine, 1 = a target with vertices but no indices or no dp, 2 = indices not strictly ascending or >= count, 3 = a delta that is
// not finite, 4 = more than 2^32 - 1 entries in total.  `where`: the target.
inline int validate_targets(const rayhip_morph_target *targets, const uint32_t targets_count, const uint32_t count, uint32_t &where) {
    uint64_t total = 0;
    for (uint32_t t = 0; t < targets_count; ++t) {
        const rayhip_morph_target &g = targets[t];
        where = t;
        if (g.count != 0 && (!g.vertices || !g.dp)) {
            return 1;
        }
        for (uint32_t k = 0; k < g.count; ++k) {
            if (g.vertices[k] >= count || (k > 0 && g.vertices[k] <= g.vertices[k - 1])) {
                return 2;
            }
            for (int i = 0; i < 3; ++i) {
                if (!rayhip_skin::finite_f(g.dp[size_t(k) * 3 + i]) || (g.dn && !rayhip_skin::finite_f(g.dn[size_t(k) * 3 + i])) ||
                    (g.db && !rayhip_skin::finite_f(g.db[size_t(k) * 3 + i]))) {
                    return 3;
                }
            }
        }
        total += g.count;
        if (total > 0xffffffffull) {
            return 4;
        }
    }
    return 0;
}

// the row table of validated targets, by counting sort: the vertices' entry counts, their prefix sums, then the targets in ascending
// order, each dropping its entries at its vertices' cursors -- which leaves every row sorted by target
inline void build_rows(const rayhip_morph_target *targets, const uint32_t targets_count, const uint32_t count, std::vector<uint32_t> &row,
                       std::vector<Entry> &entries) {
    row.assign(size_t(count) + 1, 0u);
    for (uint32_t t = 0; t < targets_count; ++t) {
        for (uint32_t k = 0; k < targets[t].count; ++k) {
            ++row[size_t(targets[t].vertices[k]) + 1];
        }
    }
    for (uint32_t v = 0; v < count; ++v) {
        row[v + 1] += row[v];
    }
    entries.assign(row[count], Entry{});
    std::vector<uint32_t> cursor(row.begin(), row.end() - 1);
    for (uint32_t t = 0; t < targets_count; ++t) {
        const rayhip_morph_target &g = targets[t];
        for (uint32_t k = 0; k < g.count; ++k) {
            Entry &e = entries[cursor[g.vertices[k]]++];
            e.target = t;
            for (int i = 0; i < 3; ++i) {
                e.dp[i] = g.dp[size_t(k) * 3 + i];
                e.dn[i] = g.dn ? g.dn[size_t(k) * 3 + i] : 0.0f;
                e.db[i] = g.db ? g.db[size_t(k) * 3 + i] : 0.0f;
            }
        }
    }
}

// plain-loop drivers over the element functions.  `used`: per vertex of the range, or null (every vertex counts).
// Return the number of used vertices whose posed position is not finite.
inline uint32_t morph_vertices_host(const rayhip_vertex *base, const uint32_t *row, const Entry *entries, const uint32_t count, const float *weights,
                                    const uint8_t *used, rayhip_vertex *out) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        morph_vertex(base[i], entries + row[i], row[i + 1] - row[i], weights, out[i]);
        bad += rayhip_skin::vertex_check(out[i], used == nullptr || used[i] != 0) ? 1u : 0u;
    }
    return bad;
}

inline uint32_t morph_skin_vertices_host(const rayhip_vertex *base, const uint32_t *row, const Entry *entries, const uint32_t count, const float *weights,
                                         const uint16_t *indices, const float *skin_weights, const float *bones, const uint8_t *used, rayhip_vertex *out) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        morph_skin_vertex(base[i], entries + row[i], row[i + 1] - row[i], weights, indices + size_t(i) * 4, skin_weights + size_t(i) * 4, bones, out[i]);
        bad += rayhip_skin::vertex_check(out[i], used == nullptr || used[i] != 0) ? 1u : 0u;
    }
    return bad;
}

} // namespace rayhip_morph
