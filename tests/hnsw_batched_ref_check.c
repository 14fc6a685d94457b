/* tests/hnsw_batched_ref_check.c -- the sequential restatement of the batched GPU HNSW builder (orc_hnsw_build_batched,
 * oracle/knn_oracle.c) as a stand-alone program, so that it can run under the host sanitizers:
 *
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ioracle \
 *      tests/hnsw_batched_ref_check.c oracle/knn_oracle.c -lm
 *
 * Three of the small configurations of tests/batched_ref.py (core-narrow, doubling-efc100, post1-d1) and the tiny graphs,
 * over rows from a linear congruential generator that tests/test_hnsw_batched_ref_cpu.py repeats: one line per
 * configuration with a hash of every list of the graph, which the test compares with the library's graph.  Last, the
 * builder resumed in the middle of a build (orc_hnsw_insert_batched) against the build with a cut there. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "knn_oracle.h"

static uint32_t lcg_state;
static uint32_t lcg(void) {
    lcg_state = (lcg_state * 1103515245u + 12345u) & 0x7fffffffu;
    return lcg_state >> 16;
}

/* coordinates k/256 in [-1, 1) */
static float* dyadic_rows(size_t n, size_t dim, uint32_t seed) {
    float* x = (float*)malloc(n * dim * sizeof(float));
    lcg_state = seed;
    for (size_t i = 0; i < n * dim; ++i) x[i] = (float)((int)(lcg() & 511u) - 256) / 256.0f;
    return x;
}

static uint64_t graph_hash(const orc_hnsw_t* g, size_t n, int maxM) {
    const int maxM0 = orc_hnsw_maxM0(g);
    int32_t* levels = (int32_t*)malloc((n + 1) * sizeof(int32_t));
    int32_t* l0 = (int32_t*)malloc((n * (size_t)(maxM0 + 1) + 1) * sizeof(int32_t));
    int32_t* up = (int32_t*)malloc((size_t)(maxM + 1) * sizeof(int32_t));
    orc_hnsw_levels(g, levels);
    orc_hnsw_links0(g, l0);
    uint64_t h = (uint64_t)orc_hnsw_maxlevel(g) * 1000003u + (uint64_t)orc_hnsw_enterpoint(g);
    for (size_t i = 0; i < n; ++i)
        for (int l = 0; l <= levels[i]; ++l) {
            const int32_t* L = l0 + i * (size_t)(maxM0 + 1);
            if (l > 0) {
                orc_hnsw_links_up(g, (int)i, l, up);
                L = up;
            }
            if (L[0] < 0 || L[0] > (l ? maxM : maxM0)) {
                fprintf(stderr, "node %zu level %d: count %d out of bounds\n", i, l, L[0]);
                exit(1);
            }
            for (int j = 0; j <= L[0]; ++j) h = h * 1000003u + (uint64_t)(uint32_t)L[j];
        }
    free(levels);
    free(l0);
    free(up);
    return h;
}

static void run(const char* name, size_t n, size_t dim, int M, int efC, int delaunay, int post, int div) {
    float* x = dyadic_rows(n, dim, 12345u);
    orc_batched_stats st;
    int32_t* batch = (int32_t*)malloc((2 * n + 2) * sizeof(int32_t));
    orc_hnsw_t* g = orc_hnsw_build_batched(ORC_L2, x, n, dim, M, M, 2 * M, efC, delaunay, post, div, 0, 0, &st, batch);
    printf("%s n=%zu hash=%llu shrinks=%lld mates=%lld\n", name, n, (unsigned long long)graph_hash(g, n, M),
           (long long)st.shrinks, (long long)st.mates);
    orc_hnsw_free(g);
    free(batch);
    free(x);
}

/* the builder resumed at `cut` on the state the build with that cut has there (orc_hnsw_insert_batched) against the build
 * with the cut itself: the same graph */
static void run_resume(const char* name, size_t n, size_t dim, int M, int efC, int delaunay, int div, size_t cut) {
    float* x = dyadic_rows(n, dim, 12345u);
    orc_batched_stats st;
    int32_t* batch = (int32_t*)malloc((2 * n + 2) * sizeof(int32_t));
    orc_hnsw_t* g = orc_hnsw_build_batched_state(ORC_L2, x, n, dim, M, M, 2 * M, efC, delaunay, div, 0, cut);
    if (orc_hnsw_insert_batched(g, 0, M, efC, delaunay, div, 0, 0, NULL, NULL) != -1 ||
        orc_hnsw_insert_batched(g, n + 1, M, efC, delaunay, div, 0, 0, NULL, NULL) != -1 ||
        orc_hnsw_insert_batched(g, cut, M, efC, delaunay, div, 0, 0, &st, batch) != 0 ||
        orc_hnsw_insert_batched(g, n, M, efC, delaunay, div, 0, 0, NULL, NULL) != 0 || /* nothing left: a no-op */
        orc_hnsw_insert_batched(g, cut, M, efC, delaunay, div, 0, 0, NULL, NULL) != -1) { /* lists are filled now */
        fprintf(stderr, "%s: orc_hnsw_insert_batched: unexpected return value\n", name);
        exit(1);
    }
    orc_hnsw_t* w = orc_hnsw_build_batched(ORC_L2, x, n, dim, M, M, 2 * M, efC, delaunay, 0, div, 0, cut, NULL, NULL);
    const uint64_t hg = graph_hash(g, n, M), hw = graph_hash(w, n, M);
    if (hg != hw) {
        fprintf(stderr, "%s: resumed graph %llu, cut build %llu\n", name, (unsigned long long)hg, (unsigned long long)hw);
        exit(1);
    }
    printf("%s n=%zu hash=%llu shrinks=%lld mates=%lld\n", name, n, (unsigned long long)hg, (long long)st.shrinks,
           (long long)st.mates);
    orc_hnsw_free(g);
    orc_hnsw_free(w);
    free(batch);
    free(x);
}

int main(void) {
    run("core-narrow", 300, 16, 6, 100, 2, 0, 0);
    run("doubling-efc100", 300, 16, 6, 100, 2, 0, 1);
    run("post1-d1", 300, 16, 6, 100, 1, 1, 0);
    for (size_t n = 1; n <= 3; ++n) run("tiny", n, 16, 6, 100, 2, 2, 0);
    run_resume("resume-at-137", 300, 16, 6, 100, 2, 0, 137);
    printf("hnsw batched restatement ok\n");
    return 0;
}
