// layering_check.cpp -- stand-alone host check of the layered-pass address mapping (Layering, rt_base.h).
//
//   layering_check W H COUNT LAYOUT [SEED]
//
// For the pass make_layering(W, H, COUNT, LAYOUT) builds, checks that (real x, real y, layer) -> packed virtual xy -> buffer index
//   * keeps both halves of the packed xy within 16 bits and the index inside the allocated virtual frame (and below 2^31),
//   * is injective,
//   * is inverted exactly by xy_layer / xy_real,
// exhaustively when the pass has at most 2^22 (pixel, layer) pairs, else on the corners of the frame and a seeded sample of 10^5 pixels
// (all layers of each).  Prints "max_layers <n>" (max_layers_for) and "ok <checked>"; a failed check prints what failed and exits 1.
// tests/test_layering_host.py compiles and runs it (and it may be built with -fsanitize=address,undefined).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../ray_amd/csrc/rt_base.h"

using namespace rt;

namespace {
int fail(const char *what, int x, int y, int layer, uint32_t xy) {
    printf("FAIL %s at x=%d y=%d layer=%d xy=%08x\n", what, x, y, layer, xy);
    return 1;
}
} // namespace

int main(int argc, char **argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: layering_check W H COUNT LAYOUT [SEED]\n");
        return 2;
    }
    const int w = atoi(argv[1]), h = atoi(argv[2]), count = atoi(argv[3]), layout = atoi(argv[4]);
    uint64_t seed = argc > 5 ? strtoull(argv[5], nullptr, 10) : 1u;
    printf("max_layers %d\n", max_layers_for(w, h, layout));
    if (count > max_layers_for(w, h, layout)) {
        printf("FAIL count above max_layers_for\n");
        return 1;
    }
    const Layering L = make_layering(w, h, count, layout);
    const int vw = virtual_width(L), rows = layer_rows(L);
    const uint64_t vsize = uint64_t(vw) * uint64_t(h) * uint64_t(rows); // elements alloc_frame gives each per-iteration buffer
    printf("cols %d rows %d virtual %d x %d\n", L.cols, rows, vw, h * rows);
    if (vsize > 0x7fffffffull) {
        printf("FAIL virtual frame of %llu elements: the pixel helpers index it with 32-bit ints\n", (unsigned long long)vsize);
        return 1;
    }
    if (uint64_t(L.cols) * uint64_t(rows) < uint64_t(count)) {
        printf("FAIL %d x %d layer slots for %d layers\n", L.cols, rows, count);
        return 1;
    }
    const uint64_t pairs = uint64_t(w) * uint64_t(h) * uint64_t(count);
    const bool exhaustive = pairs <= (uint64_t(1) << 22);
    std::vector<uint8_t> seen(exhaustive ? size_t(vsize) : 0u, 0);
    uint64_t checked = 0;
    auto check_pixel = [&](const int x, const int y, std::vector<uint64_t> *indices) {
        for (int layer = 0; layer < count; ++layer) {
            const uint32_t real = (uint32_t(x) << 16) | uint32_t(y);
            const uint32_t xy = layer_xy(L, real, uint32_t(layer));
            const uint64_t xv = xy >> 16, yv = xy & 0xffffu;
            // (the halves are 16 bits by construction of the packed form: what can go wrong is a carry from the low into the high half,
            // which shows as a coordinate outside the virtual frame or a failed inversion)
            if (xv >= uint64_t(vw) || yv >= uint64_t(h) * uint64_t(rows) || xv > 65535u || yv > 65535u) {
                return fail("virtual xy outside the frame", x, y, layer, xy);
            }
            const uint64_t idx = yv * uint64_t(vw) + xv; // rt_pixel.h: y * img_w + x
            if (idx >= vsize) {
                return fail("index outside the allocation", x, y, layer, xy);
            }
            if (count > 1 || layer == 0) {
                const uint32_t l2 = xy_layer(xy, L);
                if (l2 != uint32_t(layer)) {
                    return fail("xy_layer", x, y, layer, xy);
                }
                if (xy_real(xy, L, l2) != real) {
                    return fail("xy_real", x, y, layer, xy);
                }
            }
            if (exhaustive) {
                if (seen[size_t(idx)]) {
                    return fail("two (pixel, layer) pairs share an index", x, y, layer, xy);
                }
                seen[size_t(idx)] = 1;
            } else if (indices) {
                indices->push_back(idx);
            }
            ++checked;
        }
        return 0;
    };
    if (exhaustive) {
        for (int y = 0; y < h; ++y) {
            for (int x = 0; x < w; ++x) {
                if (check_pixel(x, y, nullptr)) {
                    return 1;
                }
            }
        }
    } else {
        // corners, then a seeded sample of distinct pixels; injectivity within the sample: sorted indices must not repeat
        std::vector<uint64_t> indices;
        std::vector<uint8_t> taken(size_t(w) * size_t(h), 0);
        const int corners[4][2] = {{0, 0}, {w - 1, 0}, {0, h - 1}, {w - 1, h - 1}};
        for (const auto &c : corners) {
            if (!taken[size_t(c[1]) * size_t(w) + size_t(c[0])]) {
                taken[size_t(c[1]) * size_t(w) + size_t(c[0])] = 1;
                if (check_pixel(c[0], c[1], &indices)) {
                    return 1;
                }
            }
        }
        for (int k = 0; k < 100000; ++k) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const uint64_t p = (seed >> 20) % (uint64_t(w) * uint64_t(h));
            if (taken[size_t(p)]) {
                continue;
            }
            taken[size_t(p)] = 1;
            if (check_pixel(int(p % uint64_t(w)), int(p / uint64_t(w)), &indices)) {
                return 1;
            }
        }
        std::sort(indices.begin(), indices.end());
        for (size_t i = 1; i < indices.size(); ++i) {
            if (indices[i] == indices[i - 1]) {
                printf("FAIL two (pixel, layer) pairs of the sample share index %llu\n", (unsigned long long)indices[i]);
                return 1;
            }
        }
    }
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
