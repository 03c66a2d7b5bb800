// Which kernel, and which instantiation of it, pam_conv2d_nhwc_bf16_ex runs a layer on: pure integer arithmetic on the call's arguments.
// Plain C++17 (no HIP header, no HIP call): the library's entry point, the layout queries, pam_conv_plan() and host-only tests share it.
// Every shape rule of the conv dispatch lives here and nowhere else; the kernels read the c3_* / KC constants below, the launchers of
// pam_conv_*.hip map a ConvPlan to a template instantiation.  What needs the device (the occupancy query behind k_conv3x3's persistent
// grid, pam_max_dynamic_lds, the PAM_C3_PERSIST_SLOTS / PAM_C3S_NBUF tuning hooks) stays in the launchers.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include "../../include/pam.h"

constexpr int KC = 64;               // K elements staged per LDS chunk of the implicit GEMMs (two 32-deep MFMA steps)
constexpr int PLAN_CUS = 256;        // the chip the rules below were measured on (MI355X); "one round of workgroups" = one per CU

// The integer arguments of pam_conv2d_nhwc_bf16_ex and which of its pointers are given (the branches check different subsets).
struct ConvQuery {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, relu, tile_cfg, in_cstride, relu_from;
    bool in, w_packed, w_img, residual, out;
};

// rc: PAM_OK or PAM_E_ARG (nothing is launched).  kernel / form: what the launch reports (PAM_CONV_KERNEL_*, the form encoding of
// include/pam.h).  The rest is what the family's launcher reads.
struct ConvPlan {
    int rc, kernel, form;
    int cin;             // k_conv3x3 / k_conv3x3s: the instantiation's input width (C3Args does not carry it)
    int ntw;             // output-channel slab of a wave / workgroup, in 16-channel tiles
    int TH;              // k_conv3x3 / k_conv3x3s: output rows per tile
    int cfg;             // k_conv3x3: M tiles per wave * 10 + waves
    int mt, pmax;        // k_conv3x3s: M tiles per multiplier wave, patch slots
    int WM, WN;          // k_conv_igemm: waves of a workgroup along pixels / channels
    int BM, NBUF;        // k_conv_gs: pixel tile, chunk ring depth
    bool gen;            // the general-activation (Darknet codes) instantiation
    bool res;            // k_conv_gs: the instantiation that carries residual rows
    bool mish;           // k_conv_gs / k_conv_stem: the instantiation whose activation is mish (code 3)
    int dbg;             // diagnostic build: k_conv3x3's knock-out / stamp bits (tile_cfg 100 .. 999)
    bool stamped;        // diagnostic build: k_conv3x3s records stamps whenever a buffer is set (pam_conv_debug_stamps)
};

inline ConvPlan plan_refused() { ConvPlan p = {}; p.rc = PAM_E_ARG; return p; }

// ---- k_conv3x3 ------------------------------------------------------------------------------------------------------------------------
// chunk of input channels resident in LDS per K pass: all 48 for Cin = 48 (K walked as the flattened (tap, c) index), 64 for the
// deep small-image layers (fewer, longer passes hide the load latency), 32 otherwise.  Pitches from tools/lds_sim.py:
// conflict-free ds_read_b128 needs pitch = 32 (mod 64) bytes for the pixel rows and these row pitches for the weights.
// widths whose instantiation carries the general (Darknet) activation epilogue; the others take codes 0 / 1 only
constexpr bool c3_general_act(int cin) { return cin == 64 || cin == 128 || cin == 256 || cin == 512; }
constexpr int c3_ck(int cin) { return cin == 48 ? 48 : (cin >= 192 ? 64 : 32); }
constexpr int c3_pitch_a(int cin) { return c3_ck(cin) == 64 ? 160 : 96; }
constexpr int c3_pitch_w(int cin) { return cin == 48 ? 864 : (c3_ck(cin) == 64 ? 1184 : 608); }

inline size_t c3_lds_bytes(int cin, int ntw, int npatch) {
    return ((((size_t)npatch + 2) * c3_pitch_a(cin) + 15) & ~(size_t)15) + (size_t)16 * ntw * c3_pitch_w(cin) + 64;
}

// choose rows per tile and the wave shape.  Measured (tools/tune_conv3x3.py): 4 M-tiles per wave beat 8, and the best
// tile is the tallest one that fits the widest block; small images take the smallest block that holds them whole.
inline void pick_rows(int H, int W, int& TH, int& cfg) {
    const int PW = W + 2;
    if (H * PW <= 128) { TH = H; cfg = 42; return; }
    if (H * PW <= 192) { TH = H; cfg = 43; return; }
    cfg = 44;
    TH = 256 / PW;
    if (TH < 1) TH = 1;
    if (TH > H) TH = H;
    // prefer a divisor of H close to the cap (no ragged last tile) when it costs < 15 % of the tile height
    for (int t = TH; t >= 1 && t * 100 >= TH * 85; --t) if (H % t == 0) { TH = t; break; }
    // wide rows (the detector's 104-wide layers): shrink the tile until its patch fits, then the block to the slots left
    while (TH > 1 && (TH + 2) * PW > 416) --TH;
    if (TH * PW <= 128 && (TH + 2) * PW <= 288) cfg = 42;
    else if (TH * PW <= 192 && (TH + 2) * PW <= 352) cfg = 43;
}

// output channels per workgroup slab of k_conv3x3 (the host packs the weight images with the same number).  The deep, small
// images (24x18, 12x9) have too few pixel tiles to fill 256 CUs, so their slabs are narrower: more, shorter workgroups.
inline int c3_slab(int H, int W, int Cin, int Cout) {
    if (Cout == 32) return 32;                                                     // HRNet-W32's 32-channel branch and transition1
    const int wide = (Cout % 48 == 0) ? 48 : 64;
    if (Cin < 192) return wide;
    if (Cout % 48 != 0) return H * W <= 1024 ? 32 : 64;                            // Darknet's 256- / 512-channel 3x3 layers
#ifdef PAM_DIAG
    const int env = getenv("PAM_C3_SLAB") ? atoi(getenv("PAM_C3_SLAB")) : 0;      // tuning hook
    if (env == 16 || env == 32 || env == 48) return env;
#endif
    return H * W <= 128 ? 16 : (H * W <= 512 ? 32 : 48);
}

// the (Cin, slab) pairs and wave shapes launch_c3() instantiates
inline bool c3_instantiated(int cin, int ntw) {
    switch (ntw) {
        case 1: return cin == 192 || cin == 384;
        case 2: return cin == 192 || cin == 384 || cin == 256 || cin == 512 || cin == 32;
        case 3: return cin == 48 || cin == 64 || cin == 96 || cin == 192 || cin == 384 || cin == 256;
        case 4: return cin == 48 || cin == 64 || cin == 96 || cin == 192 || cin == 384 || cin == 128 || cin == 256 || cin == 512;
    }
    return false;
}
inline bool c3_wave_shape(int cin, int cfg) { return cfg == 42 || cfg == 43 || cfg == 44 || (cfg == 54 && (cin == 96 || cin == 192)); }

// ---- k_conv3x3s -----------------------------------------------------------------------------------------------------------------------
// Which layers the streamed kernel takes, and its tile.  The register tile of a multiplier wave sets the LDS traffic per MFMA
// ((MT + NTW) fragment reads per MT * NTW MFMAs): with 32-channel slabs the four multipliers' reads take 75-85 % of the LDS cycles of
// their MFMAs and a chunk runs at half the matrix rate; slabs of 64 channels halve that and give the same latency
// from HALF the workgroups (120-160 at 20 crops), which leaves the other CUs to the other branches' kernels.  One workgroup per CU
// (LDS ring): the tile is the tallest whole-row tile that fits (a divisor of H when that costs < 15 %).
// Cin 96 stays on k_conv3x3: its streamed form (96-channel slabs, 160 workgroups) is as fast alone (12.9 vs 13.0 us) but 3-5 % slower
// end to end -- a 150 KB workgroup shuts the other branches out of its CU, and the 48 x 36 layers have enough tiles to fill the chip.
// c96_slab: 0 = 96 -> 96 layers stay on k_conv3x3; 48 = they run here with 48-channel slabs and a two-slot ring (the caller states it per
// launch: tile_cfg -5 of pam_conv2d_nhwc_bf16_ex, and packs the weight image for that slab: pam_conv3x3_layout_ex)
inline bool c3s_pick(int H, int W, int Cin, int Cout, int& TH, int& mt, int& pmax, int& ntw, int c96_slab = 0) {
    // layer1 / transition1 of HRNet (64 -> 64 and 256 -> 48 at 96 x 72: ReLU layers; the detector's 64- and 256-channel 3x3 layers have
    // other widths and a leaky activation and stay on k_conv3x3): two rounds of 480 workgroups, still 24 -> 16 us and 59 -> 30 us
    const bool l1 = (Cin == 64 && Cout == 64) || (Cin == 256 && Cout == 48);
    const bool c96 = Cin == 96 && Cout == 96 && c96_slab == 48;
    if (Cin != 192 && Cin != 384 && !l1 && !c96) return false;
#ifdef PAM_DIAG
    static const int mask = getenv("PAM_C3S_MASK") ? atoi(getenv("PAM_C3S_MASK")) : 14;      // tuning hook: 2 = Cin 192, 4 = 384, 8 = 64 / 256
    if (!(mask & (Cin == 192 ? 2 : (Cin == 384 ? 4 : 8)))) return false;
#endif
    const int PW = W + 2, smax = 320, pcap = l1 ? 448 : 384;
    // rows per tile: the height that costs the fewest M tiles over the image (a tile always multiplies whole 64-slot wave shares, 3 to
    // 5 of them, and a ragged last tile multiplies as much as a full one); ties go to the taller tile = fewer workgroups
    TH = 0; mt = 0; pmax = 0;
    long best = 0;
    for (int t = (H < smax / PW ? H : smax / PW); t >= 1; --t) {
        const int sl = t * PW, np = (t + 2) * PW;
        if (np > pcap) continue;
        // the instantiated (M tiles per wave, patch slots) shapes: (3, 192), (4, 320), (5, 384 | 448) -- the smallest that holds the tile
        if (sl > 320 || np > 448) continue;
        const int m = (sl <= 192 && np <= 192) ? 3 : ((sl <= 256 && np <= 320) ? 4 : 5);
        const long cost = (long)((H + t - 1) / t) * m;
        if (TH == 0 || cost < best) { TH = t; best = cost; mt = m; pmax = m == 3 ? 192 : (m == 4 ? 320 : (np <= 384 ? 384 : 448)); }
    }
    if (TH < 1) return false;
    const int bn = c96 ? c96_slab : (Cout == 48 ? 48 : 64);
    if (Cout % bn != 0) return false;
    ntw = bn / 16;
    if (c96) return true;
    // only shapes launch_c3s() instantiates: 64-channel slabs for Cin 192 / 384 (and 64 -> 64), the 48-channel slab for 256 -> 48;
    // anything else (e.g. Cin 192 -> Cout 48) stays on k_conv3x3 / the implicit GEMM and keeps the classic weight image
    if (Cin == 256 ? ntw != 3 : ntw != 4) return false;
    return true;
}
// Darknet's 3x3 layers (leaky activation, shortcut added after it) on the streamed kernel: Cin 128 / 256 / 512 with 64-channel slabs, for
// the (M tiles, patch) shapes instantiated; anything else stays on the classic kernel.  Round 5: the detector's 29 such layers ran
// at 12-17 % of the MFMA roof on k_conv3x3 (26 / 18.6 / 27.5 us at 52 x 52 / 26 x 26 / 13 x 13 x 5 views).
inline bool c3s_pick_gen(int H, int W, int Cin, int Cout, int& TH, int& mt, int& pmax) {
    if ((Cin != 128 && Cin != 256 && Cin != 512) || Cout % 64 != 0) return false;
    const int PW = W + 2;
    TH = 0; mt = 0; pmax = 0;
    long best = 0;
    for (int t = (H < 320 / PW ? H : 320 / PW); t >= 1; --t) {
        const int sl = t * PW, np = (t + 2) * PW;
        if (sl > 320 || np > 384) continue;
        const int m = (sl <= 256 && np <= 320) ? 4 : 5;
        const long cost = (long)((H + t - 1) / t) * m;
        if (TH == 0 || cost < best) { TH = t; best = cost; mt = m; pmax = m == 4 ? 320 : 384; }
    }
    return TH >= 1;
}
// slab width of the general-activation form: 64 channels for Cin = 128 (52 x 52 maps: 220 workgroups), 32 for the deeper, smaller maps
// (26 x 26, 13 x 13: 80-120 workgroups of 64-channel slabs left most of the chip idle while each streamed 300-590 KB of weights)
inline int c3s_gen_slab(int Cin) { return Cin == 128 ? 64 : 32; }

// what the weight-image layout queries of include/pam.h answer
inline int c3s_layout(int H, int W, int Cin, int Cout, int c96_slab) {
    int th, mt, pmax, ntw;
    return c3s_pick(H, W, Cin, Cout, th, mt, pmax, ntw, c96_slab) ? 16 * ntw : 0;
}
inline int c3s_layout_gen(int H, int W, int Cin, int Cout) {
    int th, mt, pmax;
    return c3s_pick_gen(H, W, Cin, Cout, th, mt, pmax) ? c3s_gen_slab(Cin) : 0;
}
// 32 = this 192- / 384-channel layer can also run with 32-channel slabs (tile_cfg -8; image packed for that width)
inline int c3s_layout_small(int H, int W, int Cin, int Cout) {
    int th, mt, pmax, ntw;
    return ((Cin == 192 || Cin == 384) && Cout % 64 == 0 && c3s_pick(H, W, Cin, Cout, th, mt, pmax, ntw, 0) && pmax != 448) ? 32 : 0;
}

// ---- k_conv_gs ------------------------------------------------------------------------------------------------------------------------
// Layers the streamed implicit GEMM takes by default (measured against k_conv_igemm per HRNet layer shape at 20 crops, tools/bench_conv.py
// --fuse --tiles=-2,8): at least two K chunks (a one-chunk tile is a load -> multiply -> store chain with nothing to overlap), and a
// tile count that suits one persistent workgroup per CU: a single round, or well-filled rounds, or a single slab (no other workgroup
// shares the gathered pixels, where k_conv_igemm's two-slab tiles would win).  270 tiles = 256 + 14 is the case to avoid: two rounds for 5 %.
inline bool conv_gs_auto(int Cout, int M, int Kpad) {
    const int bn = Cout % 48 == 0 ? 48 : 64, nslab = Cout / bn, tiles = ((M + 255) / 256) * nslab;
    if (Kpad < 128) return false;
#ifdef PAM_DIAG
    static const int mode = getenv("PAM_GS") ? atoi(getenv("PAM_GS")) : 1;                // tuning hook: 0 = never, 2 = always
    if (mode != 1) return mode == 2;
#endif
    const int rounds = (tiles + PLAN_CUS - 1) / PLAN_CUS;
    return nslab == 1 || tiles <= PLAN_CUS || tiles * 100 >= rounds * PLAN_CUS * 78;
}
// the smallest pixel tile that still is ONE round of workgroups, else 256: small layers are latency chains of a few workgroups
inline int gs_one_round_tile(int M, int nslab) {
    if (((M + 63) / 64) * nslab <= PLAN_CUS) return 64;
    if (((M + 127) / 128) * nslab <= PLAN_CUS) return 128;
    return 256;
}
inline ConvPlan plan_gs(int ntw, int BM, int NBUF, bool res, bool mish = false) {
    if (ntw >= 6 && res) return plan_refused();          // the wide slab has no registers left for the residual rows
    ConvPlan p = {};
    p.kernel = PAM_CONV_KERNEL_GS; p.form = NBUF * 1000000 + BM * 1000 + (mish ? 500 : 0) + 16 * ntw;
    p.ntw = ntw; p.BM = BM; p.NBUF = NBUF; p.res = res; p.mish = mish;
    return p;
}

// ---- k_conv_igemm ---------------------------------------------------------------------------------------------------------------------
// tile choice: share the staged input tile between two N tiles when there are two; otherwise 128-pixel blocks while they still
// give the chip >= 2 workgroups per CU, else 64-pixel blocks.  force >= 0 names one tile shape (tile_cfg 0 .. 7).
inline ConvPlan plan_igemm(int ntw, int Cout, int M, bool gen, int force) {
    const int nb = Cout / (16 * ntw);                   // N tiles of one wave
    auto blocks = [&](int wm, int wn) { return (long)((M + 64 * wm - 1) / (64 * wm)) * (nb / wn); };
    int cfg = force;
    if (cfg < 0 && ntw == 2) {
        // layers whose width is a multiple of 32 but of neither 48 nor 64 (HRNet-W32): one 32-channel N tile per wave (BN = 32); their
        // N-tile count is odd, so a workgroup is one wave wide -- 128-pixel blocks while they give the chip >= 2 workgroups per CU, else 64
        cfg = blocks(2, 1) >= 512 ? 2 : 0;
    } else if (cfg < 0) {                               // measured per HRNet layer shape with tools/bench_conv.py --tiles=...
        // 48-wide N tiles, 3 or 4 of them: the whole layer per pixel tile, the gathered input staged ONCE (merged fuse-layer heads
        // 48 -> 144 / 192, stride 2: 33.6 -> 25.4 us, 28.5 -> 25.9 us at 20 crops; 6 tiles: no gain over two workgroups of 3)
        if (ntw == 3 && nb == 3) cfg = 5;
        else if (ntw == 3 && nb == 4) cfg = 6;
        else if (nb % 2 == 0) cfg = blocks(2, 2) >= 400 ? 3 : 1;   // two N tiles per workgroup: the input tile is staged once for both
        else cfg = blocks(2, 1) >= 512 ? 2 : 0;
    }
    static const int wm_of[8] = {1, 1, 2, 2, 4, 1, 1, 2}, wn_of[8] = {1, 2, 1, 2, 1, 3, 4, 3};
    if (cfg > 7 || (ntw == 2 && cfg != 0 && cfg != 2) || nb % wn_of[cfg] != 0) return plan_refused();
    if ((long long)M * wn_of[cfg] >= (1ll << 32)) return plan_refused();      // grid.x * block.x = M * WN threads: a launch takes fewer than 2^32
    ConvPlan p = {};
    p.kernel = PAM_CONV_KERNEL_IGEMM; p.ntw = ntw; p.WM = wm_of[cfg]; p.WN = wn_of[cfg]; p.gen = gen;
    p.form = (gen ? 1000000 : 0) + 64 * p.WM * 1000 + 16 * ntw * p.WN;
    return p;
}

// ---- the streamed 3x3 kernel's stated forms ---------------------------------------------------------------------------------------------
inline ConvPlan plan_c3s(int cin, int ntw, int TH, int mt, int pmax, bool gen, bool stamped) {
    ConvPlan p = {};
    p.kernel = PAM_CONV_KERNEL_3X3S; p.form = (gen ? 100000 : 0) + cin * 100 + ntw * 10 + mt;
    p.cin = cin; p.ntw = ntw; p.TH = TH; p.mt = mt; p.pmax = pmax; p.gen = gen; p.stamped = stamped;
    return p;
}
inline bool c3_whole_tensor(const ConvQuery& q) {       // a 3x3 / stride 1 / pad 1 layer over an unsliced input, activation on every channel
    return q.KH == 3 && q.KW == 3 && q.stride == 1 && q.pad == 1 && q.in_cstride == q.Cin && q.relu_from == 0;
}
inline bool c3_out_32bit(const ConvQuery& q) { return (size_t)q.N * q.H * q.W * q.Cout * 2 < (1ull << 31); }

// ---- where each family's address arithmetic ends (DESIGN.md section 10v has the table these rest on) -------------------------------------
// Input through a buffer resource with a 32-bit byte offset, padding taps as OOB_OFFSET = 2^31 (k_conv_igemm, k_conv3x3, k_conv_stem), or
// through an int byte offset (k_conv_gs): right while the (sliced) input ends below byte 2^31 -- from there the padding offset lies INSIDE
// the resource and a padding tap reads data.  k_conv3x3s forms its input addresses as 64-bit pointers and takes any size.
inline size_t conv_in_bytes(const ConvQuery& q) { return (size_t)q.N * q.H * q.W * q.in_cstride * 2; }
inline bool conv_in_32bit(const ConvQuery& q) { return conv_in_bytes(q) < (1ull << 31); }
// k_conv_igemm without a padding tap (pad 0) and without a K tail (KH KW Cin a multiple of KC) forms OOB_OFFSET only for pixel rows past M,
// which it never stores: its input is right up to 2^32 bytes, where the offsets and num_records wrap
inline bool conv_in_igemm(const ConvQuery& q) {
    return conv_in_32bit(q) || (q.pad == 0 && (q.KH * q.KW * q.Cin) % KC == 0 && conv_in_bytes(q) < (1ull << 32));
}
// Residual rows through a buffer resource with a 32-bit byte offset in every family (OOB_OFFSET only for rows that are never stored): right
// below 2^32 bytes, where num_records and the offsets wrap.  Every family stores its output through a 64-bit pointer.
inline bool conv_res_32bit(const ConvQuery& q, int Ho, int Wo) { return !q.residual || (size_t)q.N * Ho * Wo * q.Cout * 2 < (1ull << 32); }
// Pixel and tile counts the launchers and kernels keep in an int: M = N Ho Wo, N H W (>= N * tiles), and the grids built from them
inline bool conv_counts_int(const ConvQuery& q, int Ho, int Wo) {
    return (size_t)q.N * q.H * q.W < (1ull << 31) && (size_t)q.N * Ho * Wo < (1ull << 31);
}
// tile_cfg -7: a Darknet layer (activation code > 1 allowed) on the streamed kernel, image packed for c3s_gen_slab (pam_conv3x3_layout_gen)
inline ConvPlan plan_c3s_gen(const ConvQuery& q) {
    int th = 0, mt = 0, pmax = 0;
    if (!q.in || !q.w_packed || !q.w_img || !q.out || q.N <= 0 || !c3_whole_tensor(q) ||
        !c3s_pick_gen(q.H, q.W, q.Cin, q.Cout, th, mt, pmax) || !c3_out_32bit(q)) return plan_refused();
    return plan_c3s(q.Cin, c3s_gen_slab(q.Cin) / 16, th, mt, pmax, true, false);
}
// tile_cfg -8: a 192- / 384-channel ReLU / linear layer on the streamed kernel with 32-channel slabs (pam_conv3x3_layout_small; same
// arithmetic; 16-channel slabs were measured too: no faster at 2-6 crops, slower from 9)
inline ConvPlan plan_c3s_small(const ConvQuery& q) {
    int th = 0, mt = 0, pmax = 0, ntw = 0;
    if (!q.in || !q.w_img || !q.out || q.N <= 0 || !c3_whole_tensor(q) || q.relu > 1 || !c3s_layout_small(q.H, q.W, q.Cin, q.Cout) ||
        !c3s_pick(q.H, q.W, q.Cin, q.Cout, th, mt, pmax, ntw, 0) || !c3_out_32bit(q)) return plan_refused();
    return plan_c3s(q.Cin, 2, th, mt, pmax, false, false);
}

// ---- the decision ---------------------------------------------------------------------------------------------------------------------
// tile_cfg: -1 automatic, w_img in the layout pam_conv3x3_layout() announces; -3 / -4: automatic like -1, but the caller STATES the
// layout of w_img (streamed / classic) instead of leaving it to pam_conv3x3_layout() at call time -- a launch recorded under one setting
// and re-issued under another must not read an image in the other layout; -5: streamed, and a 96 -> 96 layer's image is packed for slabs
// of 48 output channels; -2: the classic kernels (k_conv3x3 / k_conv_igemm; k_conv_gs for the detector's leaky layers), automatic
// tiles; -7 / -8: above; any other negative code: the classic kernels without k_conv_gs; 0 .. 7: one k_conv_igemm tile; 8 .. 12: k_conv_gs
// forms; >= 100: k_conv3x3 tuning hooks (1000 + TH*100 + cfg; diagnostic build also 100 + dbg bits), which refuse instead of falling back.
inline ConvPlan conv_plan(const ConvQuery& query) {
    ConvQuery q = query;
    if (q.in_cstride <= 0) q.in_cstride = q.Cin;
    if (q.in_cstride < q.Cin || q.in_cstride % 8 != 0 || q.relu_from < 0 || q.relu_from % 16 != 0) return plan_refused();
    if (q.tile_cfg == -7) return plan_c3s_gen(q);
    if (q.tile_cfg == -8) return plan_c3s_small(q);
    const int c96_slab = q.tile_cfg == -5 ? 48 : 0;
    const bool force_streamed = q.tile_cfg == -3 || c96_slab != 0, no_streamed = q.tile_cfg == -4;
    int tile_cfg = (force_streamed || no_streamed) ? -1 : q.tile_cfg;
    bool w_img = q.w_img;
    if (q.in_cstride != q.Cin || q.relu_from != 0) { if (force_streamed) return plan_refused(); w_img = false; }   // sliced input / partial activation: generic kernel only
    const int Cin = q.Cin, Cout = q.Cout, KH = q.KH, KW = q.KW, relu = q.relu;
    const bool stem = w_img && Cin == 8 && KH == 3 && KW == 3 && q.pad == 1 && !q.residual && tile_cfg < 0;
    const bool stem32 = stem && Cout == 32 && q.stride <= 2;
    // Cout % 32 == 0 only (HRNet-W32's 32-channel outputs and the 224-channel merged up-convolution): k_conv3x3<32 | 256, 2> or the
    // implicit GEMM with 32-channel slabs, below
    const bool out32 = Cout % 48 != 0 && Cout % 64 != 0 && !stem32;
    if (!q.in || !q.w_packed || !q.out || q.N <= 0 || q.H <= 0 || q.W <= 0 || Cin % 8 != 0 || (out32 && Cout % 32 != 0) ||
        KH < 1 || KW < 1 || KH > 3 || KW > 3 || q.stride < 1)
        return plan_refused();
    const int Ho = (q.H + 2 * q.pad - KH) / q.stride + 1, Wo = (q.W + 2 * q.pad - KW) / q.stride + 1;
    if (q.H >= 32768 || q.W >= 32768 || Ho < 1 || Wo < 1) return plan_refused();
    // the addressing frontiers: counts that the kernels keep in an int, the residual's 32-bit offsets (every family); the input's per family below
    if (!conv_counts_int(q, Ho, Wo) || !conv_res_32bit(q, Ho, Wo)) return plan_refused();
    const bool in32 = conv_in_32bit(q);
    const int Kpad = (KH * KW * Cin + KC - 1) / KC * KC, M = q.N * Ho * Wo;

    // k_conv_stem: w_img = the pre-permuted A fragments (see pam.h)
    if (stem && (Cout == 64 || Cout == 32) && (q.stride == 1 || q.stride == 2)) {
        const bool mish = (relu & 3) == 3;               // YOLOv4's layer 0: the stride-1 forms have a mish instantiation
        if ((mish && q.stride != 1) || !in32) return plan_refused();
        ConvPlan p = {};
        p.kernel = PAM_CONV_KERNEL_STEM; p.form = (mish ? 1000 : 0) + q.stride * 100 + Cout; p.ntw = Cout / 16; p.mish = mish;
        return p;
    }

    const bool rows3x3 = w_img && KH == 3 && KW == 3 && q.stride == 1 && q.pad == 1;
    if (force_streamed && !rows3x3) return plan_refused();
    if (rows3x3 && tile_cfg == -1 && !no_streamed) {
        // streamed kernel (specialised loader / multiplier waves): w_img then has the layout pam_conv3x3_layout() > 0 announces.
        // Any other tile_cfg (-2 = classic kernel, >= 100 = tuning hooks) takes the classic kernel and the classic images.
        int th = 0, mt = 0, pmax = 0, ntw = 0;
        const bool picked = c3s_pick(q.H, q.W, Cin, Cout, th, mt, pmax, ntw, c96_slab);
        if (force_streamed && !picked) return plan_refused();
        if (picked) return relu > 1 ? plan_refused() : plan_c3s(Cin, ntw, th, mt, pmax, false, true);
    }

    // every family from here on reaches its input with 32-bit offsets: k_conv3x3 (pad 1) and k_conv_gs (gs_ok) below 2^31 bytes; the implicit
    // GEMM takes over from k_conv_gs up to 2^32 where it forms no padding offset, and nothing takes over from it
    if (!conv_in_igemm(q)) return plan_refused();
    const bool classic = tile_cfg == -2;                 // -2: the classic kernels (k_conv3x3 / k_conv_igemm), automatic tiles
    if (classic) tile_cfg = -1;
    if (rows3x3 && (tile_cfg < 0 || tile_cfg >= 100) &&
        (Cin == 48 || Cin == 64 || Cin == 96 || Cin == 192 || Cin == 384 || Cin == 128 || Cin == 256 || Cin == 512 || (Cin == 32 && Cout == 32))) {
        const bool hook = tile_cfg >= 100;               // the tuning hooks refuse where the automatic choice falls to the generic kernel
        const int ntw = c3_slab(q.H, q.W, Cin, Cout) / 16;
        int th = 0, cfg = 0;
        pick_rows(q.H, q.W, th, cfg);
        if (tile_cfg >= 1000) { th = (tile_cfg - 1000) / 100; cfg = (tile_cfg - 1000) % 100; }
        // a row wider than the block's output slots (W + 2 > 256: the detector's 64-channel layers from 512 x 512 inputs, e.g. 304 x 304
        // at 608) or than the patch in LDS (e.g. the detector's 208-wide layers) does not fit: the generic kernel below takes it
        const int npatch = (th + 2) * (q.W + 2), pmax = (cfg == 44 || cfg == 54) ? 416 : (cfg == 43 ? 352 : 288);
        const bool fits = th * (q.W + 2) <= 16 * (cfg / 10) * (cfg % 10) && npatch <= pmax && c3_lds_bytes(Cin, ntw, npatch) <= 150 * 1024 &&
                          Cout % (16 * ntw) == 0 && (relu <= 1 || (c3_general_act(Cin) && (relu & 3) != 3));   // no mish (code 3) here: PoseResNet launches these widths' instantiations too
        if (fits && c3_instantiated(Cin, ntw)) {
            if (!c3_wave_shape(Cin, cfg)) return plan_refused();
            ConvPlan p = {};
            p.kernel = PAM_CONV_KERNEL_3X3; p.form = Cin * 10 + ntw;
            p.cin = Cin; p.ntw = ntw; p.TH = th; p.cfg = cfg;
            if (tile_cfg >= 100 && tile_cfg < 1000) p.dbg = tile_cfg - 100;
            return p;
        }
        if (hook) return plan_refused();                 // no instantiation for this (Cin, slab) or tile: generic kernel below
    }
    if (tile_cfg >= 100) tile_cfg = -1;
    const bool gen = relu > 1;                           // Darknet activation codes: the general-epilogue instantiation
    if (out32) return plan_igemm(2, Cout, M, gen, tile_cfg);

    // streamed implicit GEMM (k_conv_gs): codes 0 / 1, taps in a 32-bit mask, whole 16-byte pieces per tap (Cin % 8 == 0)
    // (round 5: code 2 -- leaky, no residual -- too: the detector's 1x1 and strided layers, which the classic implicit GEMM ran at 20 us each)
    // (code 3 -- mish, no residual -- on the 64-channel-slab forms' mish instantiations: YOLOv4's backbone)
    const bool leaky_gs = (relu == 2 || (relu == 3 && Cout % 48 != 0)) && !q.residual && classic && q.relu_from == 0;
    const bool gs_ok = (relu <= 1 || leaky_gs) && KH * KW <= 9 && Cin % 8 == 0 && (size_t)q.N * q.H * q.W * q.in_cstride * 2 < (1u << 31);
    const int slab = Cout % 48 == 0 ? 3 : 4;             // 48-channel slabs where the width allows, else 64 (Darknet's widths)
    if (leaky_gs && gs_ok && tile_cfg == -1 && conv_gs_auto(Cout, M, Kpad))
        return plan_gs(slab, slab == 4 ? gs_one_round_tile(M, Cout / 64) : 256, 3, false, relu == 3);
    if (tile_cfg >= 8 && tile_cfg <= 12 && !gs_ok) return plan_refused();
    if (tile_cfg >= 10 && tile_cfg <= 12) {
        // 12: 64-pixel tiles: the smallest images (12 x 9) as a few hundred short workgroups
        // 10 / 11: 128-pixel tiles, ring of 5 (10) / 3 (11) chunks: twice the workgroups, deeper prefetch
        if (q.residual || Cout % 48 != 0) return plan_refused();
        return plan_gs(3, tile_cfg == 12 ? 64 : 128, tile_cfg == 10 ? 5 : 3, false);
    }
    if (tile_cfg == 9)                                   // streamed implicit GEMM with 96-channel slabs: the gathered pixel tile feeds twice the MFMAs
        return Cout % 96 == 0 ? plan_gs(6, 256, 3, q.residual) : plan_refused();
    // large-M strided layers with whole 96-channel slabs and no residual (merged fuse heads 48 -> 96 / 192 at 96 x 72, transition1's
    // 256 -> 96): the 96-channel-slab form gathers every pixel tile half as often (26.3 -> 23.3, 16.2 -> 13.2, 46.2 -> 31.4 us at 20 crops;
    // slower below ~100 pixel tiles, where the layer is a latency chain whatever its tile)
    if (gs_ok && tile_cfg == -1 && !classic && !q.residual && Cout % 96 == 0 && KH == 3 && q.stride == 2 && M >= 100 * 256)
        return plan_gs(6, 256, 3, false);
    if (gs_ok && (tile_cfg == 8 || (tile_cfg == -1 && !classic && conv_gs_auto(Cout, M, Kpad)))) {
        // the small fuse-layer convolutions are latency chains of a few workgroups: the smallest pixel tile that still is ONE round of
        // workgroups (<= 256) -- at 20 crops 192 -> 384 at 12 x 9 21.3 -> 16.9 us, 48 -> 48 at 24 x 18 10.0 -> 6.1 us, 384 -> 336 1x1
        // 8.8 -> 5.8 us; two rounds lose (tools/bench_conv.py --fuse --tiles=-1,11,12)
        const int bm = (tile_cfg == -1 && !q.residual && slab == 3) ? gs_one_round_tile(M, Cout / 48) : 256;
        return plan_gs(slab, bm, 3, q.residual);
    }
    return plan_igemm(slab, Cout, M, gen, tile_cfg);
}
