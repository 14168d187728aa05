// multi_route_sanitize.cpp -- a stand-alone walk over the grids of tests/test_multi_route_model.py (every route, the pool
// shapes, the scratch layouts) for a run under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all multi_route_sanitize.cpp -o multi_route_sanitize && ./multi_route_sanitize
// It checks only what needs no second opinion (the invariants the kernels rely on); the values are the Python test's.
// TEST INFRASTRUCTURE ONLY.
#include <stdio.h>

#include "multi_route_model.cpp"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    long routes = 0, shapes = 0, layouts = 0;
    for (int form = 0; form < 6; form++)
        for (int refuse = 0; refuse < 2; refuse++)
            for (int layout = 0; layout < 6; layout++)
                for (int fits = 0; fits < 2; fits++)
                    for (int sw = 0; sw < 32; sw++) {
                        int32_t out[5];
                        mr_route(form, refuse, layout, 150, fits, sw, out);
                        CHECK(out[0] >= CAH_MULTI_SEQUENTIAL && out[0] <= CAH_MULTI_STREAM);
                        routes++;
                    }
    const int64_t PAGE = CAH_M2_PAGE;
    for (int64_t Ag : {1, 8, 96, 128})
        for (int64_t cnt : {(int64_t)1, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)1000000, (int64_t)1 << 30})
            for (int n_cus : {1, 256}) {
                const int64_t floor_cap = mr_pair_cap(1, Ag, cnt, 1), worst = mr_pages_worst(Ag, cnt);
                const int64_t lo = mr_pool_pages(floor_cap);
                for (int64_t max_pages : {lo, (lo + worst) / 2, worst})
                    for (int ungated = 0; ungated < 2; ungated++) {
                        int64_t sh[4];
                        mr_pool_shape(Ag, cnt, max_pages, n_cus, ungated, sh);
                        const int64_t n_tiles = (cnt + 1023) / 1024;
                        CHECK(sh[0] >= 1 && sh[0] <= n_cus && sh[2] >= 1);
                        if (ungated) CHECK(sh[2] == 1);
                        else if (sh[1] != max_pages) {
                            CHECK(sh[1] + sh[0] * mr_block_reserve(Ag) <= max_pages);
                            const int64_t sure = std::max<int64_t>(1, (sh[1] - sh[0] * 16 * CAH_M2_PAIR_CLASSES) / mr_pages_per_tile(Ag));
                            CHECK(sh[2] * sure >= n_tiles);
                        }
                        const int32_t counts[3] = {(int32_t)Ag, 8, (int32_t)Ag};
                        (void)mr_one_launch_for_all(counts, 3, cnt, max_pages, n_cus, ungated);
                        (void)mr_one_launch_for_all(counts, 1, cnt, max_pages, n_cus, ungated);
                        shapes++;
                    }
            }
    for (int64_t cap : {(int64_t)1, (int64_t)4095, ((int64_t)1 << 31) - 4 * PAGE})
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)100000000}) {
            uint64_t off[6];
            CHECK(mr_scratch(cap, n, off) != 0);
            for (int i = 0; i < 5; i++) CHECK(off[i] <= off[i + 1]);
            layouts++;
        }
    printf("multi_route_sanitize: %ld routes, %ld pool shapes, %ld scratch layouts: clean\n", routes, shapes, layouts);
    return 0;
}
