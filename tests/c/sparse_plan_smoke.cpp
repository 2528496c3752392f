// csrc/nwe_plan.cpp asked directly, without the library: plan_sparse, the chunks and the scratch layout of a sparse frame, which the
// ABI reaches only with a device context.  Built with the host compiler and run by tests/test_plan_host.py.  Takes triples
// n_rays S hook from its arguments or, without arguments, from stdin; prints one line per triple, the fields in the order of KEYS there.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "nwe_plan.h"

static void print(int64_t n_rays, int S, int hook) {
    const nwe::SparsePlan p = nwe::plan_sparse(n_rays, S, hook);
    const int64_t fields[] = {p.cap, p.chunks, p.M, p.at_grid, p.at_rows, p.at_z, p.at_points, p.at_dirs, p.at_offsets, p.at_total, p.at_mask, p.bytes};
    for (const int64_t f : fields) printf("%" PRId64 " ", f);
    printf("\n");
}

int main(int argc, char** argv) {
    if ((argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: sparse_plan_smoke [n_rays S hook]...   (without arguments: the triples from stdin)\n");
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) print(strtoll(argv[i], nullptr, 10), atoi(argv[i + 1]), atoi(argv[i + 2]));
    long long n_rays = 0;
    int S = 0, hook = 0;
    while (argc == 1 && scanf("%lld %d %d", &n_rays, &S, &hook) == 3) print(n_rays, S, hook);
    return 0;
}
