// Host-code hygiene of the cloud goal's host arithmetic (csrc/cloud_goal_host.h): the parameter checks of drp_set_goal_cloud, the
// limits of the predicted cloud, the eps table of the Sinkhorn kind, the mapping of a session's rows to its start columns and
// the one-shot's counts.  A stand-alone program for the host sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cloud_goal_host_check.cpp \
//       -o build/cloud_goal_host_check && build/cloud_goal_host_check
//   (or hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all ...)
//
// Every array is a heap block of exactly the size the functions may read or write, so a read or write past an end is the
// sanitizer's finding.  No device is touched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../dyn_res_pile_manip_amd/csrc/cloud_goal_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

using namespace cloud_goal;

int main() {
    const Limits lim{4096, 1024, 1000};         // KC_MAX_POINTS, KT_MAX_POINTS, KT_MAX_ITERS
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    char msg[160];

    // kinds and caps
    EXPECT(kind_ok(CHAMFER) && kind_ok(SINKHORN) && !kind_ok(2) && !kind_ok(-1));
    EXPECT(point_cap(CHAMFER, lim) == 4096 && point_cap(SINKHORN, lim) == 1024 && point_cap(7, lim) == 0);

    // parameters: what is served at the edges, what is refused just beyond them, and that a message is always written and ends
    EXPECT(check_params(CHAMFER, 1.0, 0.0, 0, 1, lim, msg, sizeof(msg)));          // eps_scale and iters are not read for Chamfer
    EXPECT(check_params(CHAMFER, 1e-300, nan, -5, 4096, lim, msg, sizeof(msg)));
    EXPECT(check_params(SINKHORN, 2.5, 1.0, 1, 1024, lim, msg, sizeof(msg)));
    EXPECT(check_params(SINKHORN, 2.5, 1e-9, 1000, 1, lim, msg, sizeof(msg)));
    struct Bad { int kind; double w, es; int it, M; const char* word; };
    const Bad bad[] = {{2, 1.0, 1.0, 10, 8, "kind"},          {-1, 1.0, 1.0, 10, 8, "kind"},         {CHAMFER, 0.0, 1.0, 10, 8, "weight"},
                       {CHAMFER, -1.0, 1.0, 10, 8, "weight"},  {CHAMFER, inf, 1.0, 10, 8, "weight"},  {CHAMFER, nan, 1.0, 10, 8, "weight"},
                       {CHAMFER, 1.0, 1.0, 10, 0, "M=0"},      {CHAMFER, 1.0, 1.0, 10, 4097, "M=4097"}, {SINKHORN, 1.0, 1.0, 10, 1025, "M=1025"},
                       {SINKHORN, 1.0, 1.0, 10, -3, "M=-3"},   {SINKHORN, 1.0, 0.0, 10, 8, "eps_scale"}, {SINKHORN, 1.0, -2.0, 10, 8, "eps_scale"},
                       {SINKHORN, 1.0, inf, 10, 8, "eps_scale"}, {SINKHORN, 1.0, nan, 10, 8, "eps_scale"}, {SINKHORN, 1.0, 1.0, 0, 8, "iters=0"},
                       {SINKHORN, 1.0, 1.0, 1001, 8, "iters=1001"}, {SINKHORN, 1.0, 1.0, -1, 8, "iters=-1"}};
    for (const Bad& b : bad) {
        std::memset(msg, 'x', sizeof(msg));
        EXPECT(!check_params(b.kind, b.w, b.es, b.it, b.M, lim, msg, sizeof(msg)));
        EXPECT(std::memchr(msg, 0, sizeof(msg)) != nullptr && std::strstr(msg, b.word) != nullptr);
        // a buffer too short for the message: truncated, terminated, nothing beyond it written
        std::vector<char> small(8, 'y');
        EXPECT(!check_params(b.kind, b.w, b.es, b.it, b.M, lim, small.data(), small.size()));
        EXPECT(small[7] == 0 || std::memchr(small.data(), 0, small.size()) != nullptr);
    }
    EXPECT(check_pred_points(CHAMFER, 4096, lim, msg, sizeof(msg)) && !check_pred_points(CHAMFER, 4097, lim, msg, sizeof(msg)));
    EXPECT(check_pred_points(SINKHORN, 1024, lim, msg, sizeof(msg)) && !check_pred_points(SINKHORN, 1025, lim, msg, sizeof(msg)));
    EXPECT(std::strstr(msg, "N=1025") != nullptr);
    EXPECT(!check_pred_points(SINKHORN, 0, lim, msg, sizeof(msg)) && !check_pred_points(9, 5, lim, msg, sizeof(msg)));

    // a target's coordinates: the first one that is no finite number, in a block of exactly M * 3 floats
    for (int M : {1, 2, 7, 341}) {
        std::vector<float> q((size_t)M * 3, 0.25f);
        EXPECT(first_nonfinite(q.data(), q.size()) == -1);
        q.back() = std::numeric_limits<float>::infinity();
        EXPECT(first_nonfinite(q.data(), q.size()) == (long)q.size() - 1);
        q[(size_t)M] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(first_nonfinite(q.data(), q.size()) == (long)M);
        q[0] = -std::numeric_limits<float>::infinity();
        EXPECT(first_nonfinite(q.data(), q.size()) == 0);
    }
    EXPECT(first_nonfinite(nullptr, 0) == -1);

    // the eps table: eps[col] = (double)eps_scale / (double)dens[col], one entry per column and none beyond
    for (int nb : {1, 2, 3, 64}) {
        std::vector<float> dens((size_t)nb);
        std::vector<double> eps((size_t)nb, -1.0);
        for (int c = 0; c < nb; ++c) dens[(size_t)c] = 125.0f * (float)(c + 1) + 0.3f;
        EXPECT(eps_table(0.7, dens.data(), nb, eps.data()) == -1);
        for (int c = 0; c < nb; ++c) EXPECT(eps[(size_t)c] == 0.7 / (double)dens[(size_t)c] && eps[(size_t)c] > 0.0);
        // the first column that gives no positive finite eps is named; the others' entries are still written
        const float poison[] = {0.0f, -3.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
        for (float v : poison) {
            std::vector<float> d2 = dens;
            d2[(size_t)(nb - 1)] = v;
            if (nb > 2) d2[1] = v;
            EXPECT(eps_table(0.7, d2.data(), nb, eps.data()) == (nb > 2 ? 1 : nb - 1));
            if (nb > 1) EXPECT(eps[0] == 0.7 / (double)dens[0]);
        }
    }
    {
        // a float density is widened before the division, not the quotient rounded: against a float division it differs
        const float d = 3.0f;
        double e = 0.0;
        EXPECT(eps_table(1.0, &d, 1, &e) == -1 && e == 1.0 / 3.0 && e != (double)(1.0f / 3.0f));
    }

    // rows to columns: row = trajectory * n_batch + column
    for (int nb : {1, 2, 5}) {
        for (long traj = 0; traj < 4; ++traj)
            for (int col = 0; col < nb; ++col) EXPECT(column_of_row(traj * nb + col, nb) == col);
        EXPECT(column_of_row(2147483646L, nb) == (int)(2147483646L % nb));
    }
    EXPECT(column_of_row(((long)1 << 40) + 3, 2) == 1);

    // the one-shot's counts
    {
        std::vector<int> n{5, 1, 5, 3};
        EXPECT(first_bad_count(nullptr, 4, 5) == -1 && first_bad_count(n.data(), 4, 5) == -1);
        n[2] = 6;
        EXPECT(first_bad_count(n.data(), 4, 5) == 2);
        n[1] = 0;
        EXPECT(first_bad_count(n.data(), 4, 5) == 1);
        n[0] = -7;
        EXPECT(first_bad_count(n.data(), 4, 5) == 0 && first_bad_count(n.data(), 0, 5) == -1);
    }

    if (failures) {
        std::printf("cloud_goal_host_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    std::printf("cloud_goal_host_check: all checks passed\n");
    return 0;
}
