// Experiment harness (not product): the tiled Fisher-Yates kernels of acav_mi.hip, each timed ALONE on synthetic draws
// (in the product they overlap on two streams and slow each other down).  Build: see tools/exp/build.sh.
#include "../../acav100m_amd/csrc/acav_mi.hip"
#include <random>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("err %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

// fy_bench mt: the generator's two kernels alone, at the product's lane block (624 * 4096 words) and its real jump polynomial
static int mt_bench()
{
    const int W = 32, reps = 20;
    const long long blk = MT_BLK_DEFAULT;
    std::mt19937 rng(5);
    std::vector<unsigned> hs((size_t)625 * W);
    for (int w = 0; w < W; ++w) {
        for (int i = 0; i < 624; ++i) hs[(size_t)w * 625 + i] = rng();
        hs[(size_t)w * 625 + 624] = 624u;
    }
    const uint32_t *g = mt_jump_poly((int64_t)W * blk);
    if (!g) { printf("no jump polynomial\n"); return 1; }
    unsigned *states, *ring, *poly;
    CK(hipMalloc(&states, 4 * hs.size())); CK(hipMemcpy(states, hs.data(), 4 * hs.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&ring, 4 * (size_t)W * blk));
    CK(hipMalloc(&poly, 4 * 624)); CK(hipMemcpy(poly, g, 4 * 624, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("MT_EPOCH %d: window of %d words, %zu B of LDS in k_mt_generate_lanes and k_mt_jump\n", MT_EPOCH, MT_WIN, sizeof(unsigned) * MT_WIN);
    auto timeit = [&](const char *name, auto fn) {
        fn(); CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < reps; ++i) fn();
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-44s %8.1f us per launch\n", name, ms * 1000.0 / reps);
    };
    for (int lanes : {1, W}) {
        char name[64];
        snprintf(name, sizeof(name), "k_mt_generate_lanes, %d lane(s) of %lld words", lanes, blk);
        timeit(name, [&]() { hipLaunchKernelGGL(k_mt_generate_lanes, dim3(lanes), dim3(MT_THREADS), 0, 0, states, ring, blk, 0ll); });
        snprintf(name, sizeof(name), "k_mt_jump, %d lane(s)", lanes);
        timeit(name, [&]() { hipLaunchKernelGGL(k_mt_jump, dim3(lanes), dim3(MT_THREADS), 0, 0, states, 0, 0, poly); });
    }
    CK(hipGetLastError());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "mt")) return mt_bench();
    const int L = argc > 1 ? atoi(argv[1]) : 1000000;
    // FYB_SLOTS=R (footprint probe, timing only): the iterations of a group share R src / g buffers (iteration z uses slot z % R)
    // instead of one each -- same launches, grids and work, wrong permutations.  Every iteration of a launch then has the same L
    // (dl = 0): an src entry written by another iteration stays inside the list, so perm and tailinv stay in range, and a g chain
    // still only descends (every g[q] < q), so the walks end.  FYB_SLOTS=16 is the unaliased layout at dl = 0 (the A/B baseline).
    const int slots = getenv("FYB_SLOTS") ? atoi(getenv("FYB_SLOTS")) : 0;
    const int G = FY_GROUP, B = 20, k = 4, dl = slots > 0 ? 0 : 4, reps = 40;
    const FyPlan fp = fy_pick_tiling(L, greedy_switches());  // the product's tiling, ACAV_FY_CAP / _TILES_MIN / _ECAP included
    printf("L %d  tiles %d cap %d gsh %d capg %d  tile smem %zu\n", L, fp.NT, fp.ecap, fp.gsh, fp.capg, fp.tile_smem());
    std::mt19937 rng(3);
    const size_t ndraw = (size_t)2 * G * L + 1024;
    std::vector<unsigned> draws(ndraw);
    for (auto &d : draws) d = rng();
    TileChunk c{};
    unsigned *dring; CK(hipMalloc(&dring, 4 * ndraw)); CK(hipMemcpy(dring, draws.data(), 4 * ndraw, hipMemcpyHostToDevice));
    c.ring = dring; c.head = 0; c.ring_words = 1ll << 62;
    unsigned short *dtab; CK(hipMalloc(&dtab, 2 * fp.table.size())); CK(hipMemcpy(dtab, fp.table.data(), 2 * fp.table.size(), hipMemcpyHostToDevice));
    int *deb; CK(hipMalloc(&deb, 4 * fp.ebound.size())); CK(hipMemcpy(deb, fp.ebound.data(), 4 * fp.ebound.size(), hipMemcpyHostToDevice));
    c.table = dtab; c.ebound = deb;
    const size_t nb = (size_t)G * fp.NT * FY_SHARDS * fp.capg, nc = (size_t)G * fp.NT * FY_SHARDS;
    CK(hipMalloc(&c.bucket, 8 * nb)); CK(hipMalloc(&c.gcount, 4 * nc)); CK(hipMemset(c.gcount, 0, 4 * nc));
    for (int q = 0; q < FY_GROUP; ++q) { CK(hipMalloc(&c.g[q], 4 * (size_t)L)); CK(hipMalloc(&c.src[q], 4 * (size_t)L)); }
    if (slots > 0 && slots < FY_GROUP) {
        for (int q = slots; q < FY_GROUP; ++q) { CK(hipFree(c.g[q])); CK(hipFree(c.src[q])); c.g[q] = c.g[q % slots]; c.src[q] = c.src[q % slots]; }
        printf("src / g: %d slots shared by the %d iterations of a group (timing only)\n", slots, FY_GROUP);
    }
    for (int q = 0; q < FY_NBUF; ++q) { CK(hipMalloc(&c.perm[q], 4 * (size_t)L)); CK(hipMemset(c.perm[q], 0, 4 * (size_t)L)); }
    CK(hipMalloc(&c.A[0], 4 * (size_t)(L + B))); CK(hipMalloc(&c.A[1], 4 * (size_t)(L + B)));
    CK(hipMemset(c.A[0], 0, 4 * (size_t)(L + B))); CK(hipMemset(c.A[1], 0, 4 * (size_t)(L + B)));
    CK(hipMalloc(&c.err, 4)); CK(hipMemset(c.err, 0, 4));
    // a tiny MI problem so that the selection in workgroup 0 runs as in the product (V = L ids, all label 0)
    const int D = 2, C = 256, P = 1;
    int *dasg, *dpairs, *dbatch, *dNc, *dac, *dbc; double *dS3, *dphi, *dG; MiScalars *dsc; long long *dS;
    CK(hipMalloc(&dasg, 4 * (size_t)L * D));
    { std::vector<int> a((size_t)L * D); for (auto &v : a) v = rng() % C; CK(hipMemcpy(dasg, a.data(), 4 * a.size(), hipMemcpyHostToDevice)); }
    int hp[2] = {0, 1}; CK(hipMalloc(&dpairs, 8)); CK(hipMemcpy(dpairs, hp, 8, hipMemcpyHostToDevice));
    CK(hipMalloc(&dbatch, 4 * 1024)); CK(hipMemset(dbatch, 0, 4 * 1024)); CK(hipMalloc(&c.tailinv, 4 * FY_NBUF * SEL_MAXB)); CK(hipMemset(c.tailinv, 0, 4 * FY_NBUF * SEL_MAXB)); CK(hipMalloc(&dNc, 4 * C * C)); CK(hipMalloc(&dac, 4 * C)); CK(hipMalloc(&dbc, 4 * C));
    CK(hipMemset(dNc, 0, 4 * C * C)); CK(hipMemset(dac, 0, 4 * C)); CK(hipMemset(dbc, 0, 4 * C));
    CK(hipMalloc(&dS3, 8 * 3)); CK(hipMemset(dS3, 0, 24));
    { std::vector<double> phi((size_t)L + 2, 0.0); for (size_t i = 1; i < phi.size(); ++i) phi[i] = (double)i * log((double)i);
      CK(hipMalloc(&dphi, 8 * phi.size())); CK(hipMemcpy(dphi, phi.data(), 8 * phi.size(), hipMemcpyHostToDevice)); }
    CK(hipMalloc(&dsc, sizeof(MiScalars))); CK(hipMemset(dsc, 0, sizeof(MiScalars)));
    const int iters = 64;
    CK(hipMalloc(&dS, 8 * iters * k)); CK(hipMalloc(&dG, 8 * iters * k));
    c.asg = dasg; c.pairs = dpairs; c.batch = dbatch; c.Nc = dNc; c.ac = dac; c.bc = dbc; c.SN = dS3; c.Sa = dS3 + 1; c.Sb = dS3 + 2;
    c.phi = dphi; c.sc = dsc; c.S = dS; c.G = dG;
    c.L0 = L; c.iters = iters; c.ntab = (int)fp.table.size(); c.gsh = fp.gsh; c.NT = fp.NT; c.capg = fp.capg; c.ecap = fp.ecap_lds; c.wcap = fp.wcap;
    c.D = D; c.C = C; c.P = P;
    TileChunk *dcd; CK(hipMalloc(&dcd, sizeof(c))); CK(hipMemcpy(dcd, &c, sizeof(c), hipMemcpyHostToDevice));
    // FYB_PACK=0: 8-byte bucket entries (the product's ACAV_FY_PACK=0)
    const bool pack = L <= FY_PACK_MAX && !(getenv("FYB_PACK") && getenv("FYB_PACK")[0] == '0');
    const auto tile_k = pack ? k_fy_tile_multi<true> : k_fy_tile_multi<false>;
    const auto part_st = pack ? k_fy_part_multi<true, true> : k_fy_part_multi<true, false>;
    const auto part_di = pack ? k_fy_part_multi<false, true> : k_fy_part_multi<false, false>;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(tile_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp.tile_smem()));
    const bool staged = getenv("FYB_PART_DIRECT") == nullptr;
    const size_t part_smem = fy_part_smem(fp.NT, fp.table.size(), staged, pack);
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(part_st), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fy_part_smem(fp.NT, fp.table.size(), true, pack)));
    printf("part: %s, %zu B of LDS; bucket entries of %d bytes\n", staged ? "staged" : "direct", part_smem, pack ? 4 : 8);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto part = [&]() { hipLaunchKernelGGL(staged ? part_st : part_di, dim3((L + FYA_CH - 1) / FYA_CH, 1, G), dim3(FYA_THREADS), part_smem, 0, dcd, 0, dl); };
    // the product's grids of the tile and resolve kernels (fy_launch_grid) under the product's switch: ACAV_FY_XCD_AFFINE=0 = 3-D
    const bool affine = !(getenv("ACAV_FY_XCD_AFFINE") && getenv("ACAV_FY_XCD_AFFINE")[0] == '0');
    FyGrid gr_tile, gr_res;
    const dim3 grid_tile = to_dim3(fy_launch_grid(affine, (unsigned)fp.NT, 1u, (unsigned)G, FYT_THREADS, &gr_tile));
    const dim3 grid_res = to_dim3(fy_launch_grid(affine, (unsigned)((L + 255) / 256), 1u, (unsigned)G, 256, &gr_res));
    printf("tile / resolve grids: %s (%u / %u workgroups in x)\n", gr_tile.nx ? "1-D, one XCD per iteration" : "3-D", grid_tile.x, grid_res.x);
    auto tile = [&]() { hipLaunchKernelGGL(tile_k, grid_tile, dim3(FYT_THREADS), fp.tile_smem(), 0, dcd, 0, dl, gr_tile); };
    auto resolve = [&]() { hipLaunchKernelGGL(k_fy_resolve_multi<false>, grid_res, dim3(256), 0, 0, dcd, 0, dl, B - k, gr_res); };
    auto timeit = [&](const char *name, auto fn, double base_us) {
        for (int i = 0; i < 3; ++i) fn();
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < reps; ++i) fn();
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        const double us = ms * 1000.0 / reps;
        printf("%-34s %8.2f us per group  (%.2f us per iteration; minus previous: %.2f)\n", name, us, us / G, (us - base_us) / G);
        return us;
    };
    const double t_ms = timeit("memset counters", [&]() { CK(hipMemsetAsync(c.gcount, 0, 4 * nc, 0)); }, 0);
    const double t_p = timeit("memset + part", [&]() { CK(hipMemsetAsync(c.gcount, 0, 4 * nc, 0)); part(); }, t_ms);
    if (getenv("FYB_ONLY_PART")) return 0;  // -DACAV_FY_ABL_BKSEQ leaves buckets the tile kernel must not read
    const double t_pt = timeit("memset + part + tile", [&]() { CK(hipMemsetAsync(c.gcount, 0, 4 * nc, 0)); part(); tile(); }, t_p);
    timeit("part + tile + resolve", [&]() { part(); tile(); resolve(); }, t_pt - t_ms);
    (void)t_ms;
#ifdef ACAV_FY_PROF
    {   // phase ticks of k_fy_tile, one group
        unsigned long long z16[16] = {0}, pr[16];
        CK(hipMemsetAsync(c.gcount, 0, 4 * nc, 0)); part(); CK(hipDeviceSynchronize());
        CK(hipMemcpyToSymbol(HIP_SYMBOL(fy_prof), z16, sizeof(z16)));
        tile(); CK(hipDeviceSynchronize());
        CK(hipMemcpyFromSymbol(pr, HIP_SYMBOL(fy_prof), sizeof(pr)));
        const double wgs = (double)fp.NT * G;
        const char *nm[5] = {"prologue (bounds, counters)", "LDS init", "entries: bucket -> lists", "walk + src scatter", "g store"};
        for (int q = 0; q < 5; ++q) printf("   tile phase %-28s %7.2f us per workgroup\n", nm[q], pr[q] / wgs / 100.0);
    }
#endif
    unsigned err; CK(hipMemcpy(&err, c.err, 4, hipMemcpyDeviceToHost)); printf("err flags %u\n", err);
    // gathers of iterations 0..G-1, alone (perm / src / g of the last group are in place)
    const int sel_m = sel_mode(B, P, k);
    const size_t sel_smem = sel_layout(B, P, D, k, sel_m).total;
    // the product's switches of the gather's XCD subset (gs_block_map): ACAV_GS_XCDS = 1, 2, 4, 8 and ACAV_GS_XCD_ROT = 0 / 1.
    // FYB_GS_PAD=n (probe, timing only): all eight classes gather, the grid padded to the length it has at ACAV_GS_XCDS=n -- what
    // the padding workgroups alone cost
    const int gs_n = getenv("ACAV_GS_XCDS") ? atoi(getenv("ACAV_GS_XCDS")) : GS_XCDS_DEFAULT;
    if (gs_n != 1 && gs_n != 2 && gs_n != 4 && gs_n != 8) { printf("ACAV_GS_XCDS: 1, 2, 4 or 8\n"); return 1; }
    const bool gs_rot = getenv("ACAV_GS_XCD_ROT") ? getenv("ACAV_GS_XCD_ROT")[0] == '1' : GS_XCD_ROT_DEFAULT;
    const int gs_pad = getenv("FYB_GS_PAD") ? atoi(getenv("FYB_GS_PAD")) : 0;
    if (gs_pad != 0 && gs_pad != 1 && gs_pad != 2 && gs_pad != 4 && gs_pad != 8) { printf("FYB_GS_PAD: 1, 2, 4 or 8\n"); return 1; }
    GsGrid gr_gs = {(unsigned)FY_XCDS, 0u};
    long long gs_launch = 0;
    auto gs_grid = [&]() {  // sets gr_gs for the launch that follows
        const long long gb = (L + 256 * GS_EPT - 1) / (256 * GS_EPT);
        if (gs_pad) return dim3((unsigned)gs_grid_blocks(gb, (unsigned)gs_pad, 0u), 1);
        gr_gs = {(unsigned)gs_n, gs_rot && gs_n < FY_XCDS ? (unsigned)(gs_launch++ * gs_n % FY_XCDS) : 0u};
        return dim3((unsigned)gs_grid_blocks(gb, gr_gs.n_xcd, gr_gs.rot), 1);
    };
    printf("gather grid: %d XCD(s), rotation %d, %u workgroups%s\n", gs_n, (int)gs_rot, gs_grid().x, gs_pad ? "  [all eight gather, padded row]" : "");
    int itg = 0;
    auto g_sc = [&]() { hipLaunchKernelGGL((k_fy_gather_select_multi<false, false>), gs_grid(), dim3(256), sel_smem, 0, dcd, itg, dl, B, k, sel_m, 1, gr_gs); itg = (itg + 1) % G; };
    timeit("G x gather+select", [&]() { for (int i = 0; i < G; ++i) g_sc(); }, 0);
    {   // iteration 0 only: no selection in workgroup 0 -- the gather alone
        auto g0only = [&]() { hipLaunchKernelGGL((k_fy_gather_select_multi<false, false>), gs_grid(), dim3(256), sel_smem, 0, dcd, 0, dl, B, k, sel_m, 1, gr_gs); };
        timeit("G x gather (launch 0: no selection)", [&]() { for (int i = 0; i < G; ++i) g0only(); }, 0);
    }
    {   // the same with ONE perm buffer for every iteration (stays in cache) -- how much of the gather is the first touch of perm?
        TileChunk c2 = c;
        for (int q = 0; q < FY_NBUF; ++q) c2.perm[q] = c.perm[0];
        CK(hipMemcpy(dcd, &c2, sizeof(c2), hipMemcpyHostToDevice));
        timeit("G x gather+select, one perm buffer", [&]() { for (int i = 0; i < G; ++i) g_sc(); }, 0);
        CK(hipMemcpy(dcd, &c, sizeof(c), hipMemcpyHostToDevice));
    }
    {   // do the two streams of the product overlap?  side group (iterations 8..15) on one stream, 8 gathers (0..7) on another
        const char *pri = getenv("FYB_PRIORITY"), *mask = getenv("FYB_CUMASK");
        hipStream_t sa, sb;
        int lo = 0, hi = 0;
        CK(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = least priority (largest number)
        if (mask) {
            const int ncu = atoi(mask);  // side stream restricted to the first ncu CUs of every XCD-interleaved mask word
            uint32_t m[8];
            for (int q = 0; q < 8; ++q) m[q] = 0;
            for (int cu = 0; cu < ncu; ++cu) m[cu / 32] |= 1u << (cu % 32);
            CK(hipExtStreamCreateWithCUMask(&sa, 8, m));
        } else {
            CK(hipStreamCreateWithPriority(&sa, hipStreamNonBlocking, pri ? lo : 0));
        }
        CK(hipStreamCreateWithPriority(&sb, hipStreamNonBlocking, pri ? hi : 0));
        auto side = [&](hipStream_t st) {
            hipLaunchKernelGGL(staged ? part_st : part_di, dim3((L + FYA_CH - 1) / FYA_CH, 1, G), dim3(FYA_THREADS), part_smem, st, dcd, 8, dl);
            hipLaunchKernelGGL(tile_k, grid_tile, dim3(FYT_THREADS), fp.tile_smem(), st, dcd, 8, dl, gr_tile);
            hipLaunchKernelGGL(k_fy_resolve_multi<false>, grid_res, dim3(256), 0, st, dcd, 8, dl, B - k, gr_res);
        };
        const bool nosel = getenv("FYB_NOSEL") != nullptr;  // every gather as launch 0: no selection beside it
        auto gath = [&](hipStream_t st) {
            for (int i = 0; i < G; ++i)
                hipLaunchKernelGGL((k_fy_gather_select_multi<false, false>), gs_grid(), dim3(256), sel_smem, st, dcd, nosel ? 0 : i, dl, B, k, sel_m, 1, gr_gs);
        };
        auto wall = [&](const char *name, auto fn) {
            fn(); CK(hipDeviceSynchronize());
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < reps; ++r) fn();
            CK(hipDeviceSynchronize());
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            printf("%-44s %8.2f us per group (%.2f us per iteration)\n", name, us, us / G);
        };
        printf("priority range %d (low) .. %d (high)%s%s\n", lo, hi, pri ? "  [side low, gathers high]" : "", mask ? "  [side CU-masked]" : "");
        wall("side group alone (stream a)", [&]() { side(sa); });
        wall("8 gathers alone (stream b)", [&]() { gath(sb); });
        wall("both, two streams", [&]() { side(sa); gath(sb); });
    }
#ifdef ACAV_FY_PROF
    {   // phase ticks of the selection in workgroup 0 of the gather kernel
        unsigned long long z16[16] = {0}, pr[16];
        CK(hipDeviceSynchronize());
        CK(hipMemcpyToSymbol(HIP_SYMBOL(fy_prof), z16, sizeof(z16)));
        for (int i = 0; i < G; ++i) g_sc();
        CK(hipDeviceSynchronize());
        CK(hipMemcpyFromSymbol(pr, HIP_SYMBOL(fy_prof), sizeof(pr)));
        const char *nm[5] = {"ids -> LDS (after the gather)", "scoring", "means + top-k", "picks + requeue", "commit"};
        for (int q = 0; q < 5; ++q) printf("   select phase %-30s %7.2f us\n", nm[q], pr[8 + q] / (double)G / 100.0);
    }
#endif
    return 0;
}
