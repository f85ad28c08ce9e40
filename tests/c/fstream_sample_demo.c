/* fstream_sample_demo.c -- a sampling, evaluating frame stream (include/vppx.h: vppx_fstream_create_sampled) from plain C: the
 * reference's loop (test.py:291-311) for a dataset without raw hints, where every frame's hints are sampled from its ground truth
 * (test.py:125-129).  The frames and the ground truth are those of fstream_eval_demo.c (same LCG); no push brings hints, src is NULL:
 * the gt the push brings anyway is what the device samples from.  Prints one line per frame: its index, the FNV-1a hash of its
 * disparity map and the eight doubles of its VppxMetrics record as 64-bit hex patterns; tests/test_gpu_sample_path.py compares them
 * with vppstereo_amd.pipeline.FrameStream(sample=..., metrics=True).
 * Build: gcc -std=c99 -O1 -I include tests/c/fstream_sample_demo.c -o demo -L vppstereo_amd -lvppx -Wl,-rpath,$PWD/vppstereo_amd
 * Usage: demo <frames> <H> <W> <dmax> <batch> <seed> <sample seed> <probability> */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vppx.h"

static uint32_t lcg_state;
static uint32_t lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }

static uint64_t fnv1a(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

#define CHECK(call)                                                                     \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ < 0) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, vppx_last_error()); return 1; } \
    } while (0)

static void print_frame(int f, const float *disp, size_t px, const VppxMetrics *m)
{
    uint64_t w[8];
    memcpy(w, m, sizeof(w));
    printf("%d %016llx", f, (unsigned long long)fnv1a(disp, px * sizeof(float)));
    for (int k = 0; k < 8; k++) printf(" %016llx", (unsigned long long)w[k]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: %s frames H W dmax batch seed sample_seed probability\n", argv[0]); return 2; }
    const int n = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), D = atoi(argv[4]), batch = atoi(argv[5]);
    const uint32_t seed = (uint32_t)strtoul(argv[6], NULL, 10);
    const size_t px = (size_t)H * W;
    uint8_t *left = malloc(px * 3), *right = malloc(px * 3);
    float *gt = malloc(px * sizeof(float)), *validgt = malloc(px * sizeof(float)), *disp = malloc(px * sizeof(float));
    vppx_ctx *ctx = NULL;
    vppx_fstream *fs = NULL;
    VppxVppParams vp;
    VppxRsgmParams rp;
    VppxOccParams op;
    VppxEvalParams ep;
    VppxSampleParams smp;
    VppxMetrics m;
    if (sizeof(VppxSampleParams) != 24) { fprintf(stderr, "struct sizes\n"); return 2; }
    CHECK(vppx_create(&ctx, -1));
    vppx_vpp_params_default(&vp);
    vppx_rsgm_params_default(&rp);
    vppx_occ_params_default(&op);
    vppx_eval_params_default(&ep);
    vppx_sample_params_default(&smp);
    vp.seed = seed;
    rp.dmax = D;
    smp.seed = (uint32_t)strtoul(argv[7], NULL, 10);
    smp.probability = atof(argv[8]);
    CHECK(vppx_fstream_create_sampled(ctx, &op, &vp, &rp, NULL, &ep, &smp, batch, 3, H, W, 3, VPPX_FS_METRICS | VPPX_FS_SAMPLE, 2, &fs));
    int popped = 0, got = 0;
    /* a sampling stream takes its frames through vppx_fstream_push_sampled only */
    if (vppx_fstream_push_eval(fs, left, right, gt, NULL, NULL, gt, validgt) != VPPX_E_INVALID_ARG) { fprintf(stderr, "push_eval was not refused\n"); return 4; }
    for (int f = 0; f < n; f++) {
        lcg_state = 12345u + 977u * (uint32_t)f;
        for (size_t i = 0; i < px * 3; i++) left[i] = (uint8_t)(lcg() >> 24);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int c = 0; c < 3; c++) {
                    const int xs = x + 5 < W ? x + 5 : W - 1;
                    right[((size_t)y * W + x) * 3 + c] = (uint8_t)(left[((size_t)y * W + xs) * 3 + c] ^ (lcg() >> 31));
                }
        for (size_t i = 0; i < px; i++) (void)lcg(); /* (the draws fstream_eval_demo.c spends on its hints) */
        for (size_t i = 0; i < px; i++) {
            const uint32_t r = lcg();
            gt[i] = 3.0f + (float)((r >> 16) & 15) * 0.25f;
            validgt[i] = (r >> 30) != 0 ? 1.0f : 0.0f;
        }
        CHECK(vppx_fstream_push_sampled(fs, left, right, NULL, NULL, NULL, gt, validgt));
        int64_t unpopped = 0;
        CHECK(vppx_fstream_counts(fs, NULL, NULL, &unpopped, NULL));
        while (unpopped > 2 * batch) {
            CHECK(vppx_fstream_pop_eval(fs, disp, NULL, NULL, NULL, NULL, &m, &got));
            if (!got) break;
            print_frame(popped++, disp, px, &m);
            unpopped--;
        }
    }
    CHECK(vppx_fstream_flush(fs));
    for (;;) {
        CHECK(vppx_fstream_pop_eval(fs, disp, NULL, NULL, NULL, NULL, &m, &got));
        if (!got) break;
        print_frame(popped++, disp, px, &m);
    }
    vppx_fstream_destroy(fs);
    vppx_destroy(ctx);
    free(left); free(right); free(gt); free(validgt); free(disp);
    return popped == n ? 0 : 3;
}
