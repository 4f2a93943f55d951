/*
 * extent_oracle.c -- the fused renderer's image at LISTED pixels of an image too large to hold.  TEST INFRASTRUCTURE.
 *
 * Follows primary_accept.c in tests/oracles.c (and with it oracle/pt_oracle.c, whole).  ptor_render folds into a W x H framebuffer,
 * 34 GB for an image of 2^31 - 1 pixels; this folds the same frames of the same ptor_sample_pixel -- the oracle's own sample and its
 * own fold (GenerateColors.cl:302-321), not a restatement of either -- into one float4 per listed pixel.  Compiled with
 * oracle/Makefile's flags (tests/oracles.py).
 */
/* px[k][4] (k < n): frames [frame_begin, frame_begin + frame_count) of pixel gid[k] of the W x H image folded, in ascending order,
 * into what px[k] holds (frame 0 starts afresh).  stats (may be NULL): the oracle's work tallies over all of them, ptor_stats_words()
 * words.  Returns -1 for a gid outside the image or a frame range beyond 2^31 - 1. */
PTOR_CLONES
int oex_render_window(const void* tris, int ntri, const void* mats, int W, int H, int frame_begin, int frame_count, int max_bounces,
                      const int32_t* gid, int64_t n, float* px, uint64_t* stats)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    if (W < 1 || H < 1 || frame_begin < 0 || frame_count < 0 || (int64_t)frame_begin + frame_count > 0x7fffffffLL) return -1;
    for (int64_t k = 0; k < n; ++k)
        if (gid[k] < 0 || (int64_t)gid[k] >= (int64_t)W * H) return -1;
    for (int64_t k = 0; k < n; ++k)
        for (int f = 0; f < frame_count; ++f)
            ptor_sample_pixel((const ptor_triangle*)tris, ntri, (const ptor_material*)mats, px + 4 * k, gid[k], W, H, frame_begin + f,
                              max_bounces, &st);
    if (stats) memcpy(stats, &st, sizeof st);
    return 0;
}
