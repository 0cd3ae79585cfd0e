// Host-code hygiene of the dataset calls (csrc/ptcl_dataset_host.h): where the blocks of the upload arena lie for
// drp_ptcl_dataset_batch and for drp_ptcl_dataset_frames, and which image a call refuses for what.  A stand-alone program for the
// host sanitizers:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/ptcl_dataset_host_check.cpp -o build/ptcl_dataset_host_check && build/ptcl_dataset_host_check
//   (or any C++17 compiler: c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all ...)
//
// The layout of both kinds of call is held to sizes summed by hand here, an independent restatement, and every block is written
// in full inside a heap block of exactly PdLayout::bytes, so a block that overlaps the next one or runs past the end is the
// sanitizer's finding.  The check functions walk crafted inputs with two faults each: the first image in index order, and its
// first fault in the documented order, is the one reported.  No device is touched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../dyn_res_pile_manip_amd/csrc/ptcl_dataset_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static size_t up(size_t v) { return (v + 255) / 256 * 256; }

// one call's arena: T = 0 the frames call over n_img = B * T images, T >= 2 the batch call with n_ptcl particles per sample
static void stage(int n_img, size_t npix, int n_ptcl, int T) {
    const size_t n = (size_t)n_img, ptcl_floats = T ? n * T * n_ptcl * 4 : 0;
    const PdLayout L = pd_layout(n_img, npix, ptcl_floats, T);
    // the blocks in their order in memory, sizes summed by hand; the frames call has the first, third and fifth only
    const size_t off[] = {L.depth, L.ptcl, L.radius, L.push, L.init, L.nptcl, L.ptcl_off, L.bytes};
    const size_t len[] = {n * npix * 2, ptcl_floats * 4, n * 8, T ? n * (T - 1) * 10 * 8 : 0, n * 4, T ? n * 4 : 0, T ? n * 8 : 0};
    size_t at = 0;
    for (int k = 0; k < 7; ++k) {
        EXPECT(off[k] == at && off[k] % 256 == 0);
        at = up(at + len[k]);
    }
    EXPECT(L.bytes == at);
    if (!T) {                                                    // depth | radius | init and not a byte more
        EXPECT(L.radius == up(n * npix * 2) && L.init == up(L.radius + n * 8) && L.bytes == up(L.init + n * 4));
        EXPECT(L.ptcl == L.radius && L.push == L.init && L.nptcl == L.bytes && L.ptcl_off == L.bytes);
    }
    char* pin = static_cast<char*>(std::malloc(L.bytes));
    std::memset(pin, 0xff, L.bytes);
    for (int k = 0; k < 7; ++k) std::memset(pin + off[k], k + 1, len[k]);
    for (int k = 0; k < 7; ++k)                                  // no block overwrote another
        if (len[k]) EXPECT(pin[off[k]] == k + 1 && pin[off[k] + len[k] - 1] == k + 1);
    std::free(pin);
}

static bool is(const PdBad& b, int img, PdFault fault, int push = 0) { return b.img == img && b.fault == fault && b.push == push; }

int main() {
    // B = 1; odd sizes; the 40 x 33 test images and a 720 x 720 frame; the most images a call takes
    const int fshapes[][2] = {{1, 1}, {1, 1320}, {6, 1320}, {3, 1}, {24, 518400}, {1024, 7}};
    for (const auto& s : fshapes) stage(s[0], (size_t)s[1], 0, 0);            // frames calls: {B * T, npix}, T = 1 among them
    const int bshapes[][4] = {{1, 1, 1, 2}, {1, 1320, 1, 2}, {3, 1320, 1, 3}, {2, 1320, 5, 2}, {64, 518400, 999, 6}, {1024, 7, 3, 2}};
    for (const auto& s : bshapes) stage(s[0], (size_t)s[1], s[2], s[3]);      // batch calls: {B, npix, n_ptcl, T}

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    {
        // the pre-launch walk, on heap arrays of exactly the documented sizes: B = 3 samples, T = 3 (two pushes each)
        const int B = 3, T = 3;
        const size_t npix = 1320;
        std::vector<double> radius(B, 0.05), push((size_t)B * (T - 1) * PD_PUSH, 0.0);
        std::vector<int32_t> init(B, 0), nfg(B, 100), nptcl(B, 5);
        for (int e = 0; e < B * (T - 1); ++e) { push[e * PD_PUSH + 6] = 1.0; push[e * PD_PUSH + 9] = 1.0; }
        auto batch = [&]() { return pd_first_bad(B, npix, radius.data(), init.data(), nfg.data(), nptcl.data(), push.data(), T); };
        auto frames = [&]() { return pd_first_bad(B, npix, radius.data(), init.data(), nfg.data()); };
        EXPECT(is(batch(), -1, PD_FINE) && is(frames(), -1, PD_FINE));
        nfg[2] = 1320;                                           // every pixel is allowed, one more is not
        EXPECT(is(batch(), -1, PD_FINE));
        nfg[2] = 1321;
        EXPECT(is(batch(), 2, PD_BAD_NFG) && is(frames(), 2, PD_BAD_NFG));
        nfg[1] = -1;                                             // an earlier image goes first
        EXPECT(is(batch(), 1, PD_BAD_NFG) && is(frames(), 1, PD_BAD_NFG));
        push[((size_t)1 * (T - 1) + 1) * PD_PUSH + 8] = 1e-6;    // within an image: the pushes before the host's count
        EXPECT(is(batch(), 1, PD_PUSH_PLANE, 1) && is(frames(), 1, PD_BAD_NFG));
        push[((size_t)1 * (T - 1) + 1) * PD_PUSH + 9] = 0.0;     // of one push: the length before the plane
        EXPECT(is(batch(), 1, PD_PUSH_LEN, 1));
        push[((size_t)1 * (T - 1) + 0) * PD_PUSH + 8] = nan;     // the pushes in their order
        EXPECT(is(batch(), 1, PD_PUSH_PLANE, 0));
        push[((size_t)1 * (T - 1) + 0) * PD_PUSH + 9] = inf;
        EXPECT(is(batch(), 1, PD_PUSH_LEN, 0));
        radius[1] = inf;                                         // the radius before the pushes
        EXPECT(is(batch(), 1, PD_BAD_RADIUS) && is(frames(), 1, PD_BAD_RADIUS));
        radius[1] = nan;
        EXPECT(is(batch(), 1, PD_BAD_RADIUS));
        radius[1] = 0.0;
        EXPECT(is(frames(), 1, PD_BAD_RADIUS));
        init[1] = -1;                                            // the start before the radius
        EXPECT(is(batch(), 1, PD_BAD_INIT) && is(frames(), 1, PD_BAD_INIT));
        nptcl[1] = 0;                                            // the particle count first, where there is one
        EXPECT(is(batch(), 1, PD_NO_PTCL) && is(frames(), 1, PD_BAD_INIT));
        push[(size_t)(B * (T - 1) - 1) * PD_PUSH + 9] = -1.0;    // the last push of the last sample: read, and nothing behind it
        nptcl[1] = 5; init[1] = 0; radius[1] = 0.05; nfg[1] = 100; nfg[2] = 7;
        for (int t = 0; t < T - 1; ++t) { push[((size_t)1 * (T - 1) + t) * PD_PUSH + 8] = 0.0; push[((size_t)1 * (T - 1) + t) * PD_PUSH + 9] = 2.0; }
        EXPECT(is(batch(), 2, PD_PUSH_LEN, 1) && is(frames(), -1, PD_FINE));
        radius[0] = -0.0;
        EXPECT(is(batch(), 0, PD_BAD_RADIUS));
    }
    {
        // the walk over the device's counts: six images (B = 2, T = 3 of a frames call), cap 4096
        const int n = 6;
        std::vector<int> nfg = {500, 300, 640, 64, 900, 1100}, counts = {40, 30, 4096, 5, 1, 77};
        std::vector<int32_t> host(nfg.begin(), nfg.end()), init = {499, 0, 3, 63, 10, 555};
        auto late = [&]() { return pd_first_bad_counts(n, nfg.data(), counts.data(), host.data(), init.data(), 4096); };
        EXPECT(is(late(), -1, PD_FINE));
        counts[5] = 4097;
        EXPECT(is(late(), 5, PD_CAPPED));
        init[5] = 1100;                                          // the start before the cap
        EXPECT(is(late(), 5, PD_INIT_OUTSIDE));
        host[5] = 1099;                                          // the host's count before the start
        EXPECT(is(late(), 5, PD_NFG_DIFFERS));
        nfg[5] = 0;                                              // an empty image before everything
        EXPECT(is(late(), 5, PD_NO_FG));
        init[3] = 64;                                            // an earlier image goes first
        EXPECT(is(late(), 3, PD_INIT_OUTSIDE));
        counts[0] = 5000;
        EXPECT(is(late(), 0, PD_CAPPED));
    }
    std::printf(failures ? "%d checks FAILED\n" : "ptcl_dataset_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
