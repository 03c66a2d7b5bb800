// What pam_fuse_sum_nhwc_bf16 accepts and what it launches for it: pure integer arithmetic on the call's arguments.
// Plain C++17 (no HIP header, no HIP call): the entry point, pam_fuse_sum_plan() and host-only tests share it.  Every shape rule of the
// fuse-layer sums lives here and nowhere else: the argument check, the table of instantiated combinations, the unit rectangle of an
// anchor level, the rule that picks kernel and level, and the persistent kernel's tile candidates and LDS layout.  pam_fuse.hip keeps
// the kernels, their argument structs and launchers; what needs the device (pam_cu_count, pam_max_dynamic_lds) stays there.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/pam.h"

constexpr int FL_MAXI = 5;                       // k_fuse_sum_lds: 16-byte items of the output tile per thread at most
constexpr int FL_LDS_MAX = 160 * 1024;           // k_fuse_sum_lds: dynamic LDS of a workgroup at most

// The integer arguments of pam_fuse_sum_nhwc_bf16 (counts as passed; of the arrays, the entries the counts name, at most 2 and 3) and
// the compute units the grid of the persistent kernel is sized by.
struct FuseQuery {
    int N, H, W, C;
    int n_plain, plain_cs[2];                    // plain_cs <= 0: C
    int n_up, shift[3], src_c[3];
    int tile_a, tile_b, max_workgroups, n_cu;
};

inline FuseQuery fuse_query(int N, int H, int W, int C, int n_plain, const int32_t* plain_cstrides, int n_up, const int32_t* up_shifts,
                            const int32_t* up_channels, int tile_a, int tile_b, int max_workgroups, int n_cu) {
    FuseQuery q = {};
    q.N = N; q.H = H; q.W = W; q.C = C; q.n_plain = n_plain; q.n_up = n_up;
    for (int t = 0; t < n_plain && t < 2; ++t) q.plain_cs[t] = plain_cstrides ? plain_cstrides[t] : 0;
    for (int s = 0; s < n_up && s < 3; ++s) { q.shift[s] = up_shifts[s]; q.src_c[s] = up_channels[s]; }
    q.tile_a = tile_a; q.tile_b = tile_b; q.max_workgroups = max_workgroups; q.n_cu = n_cu;
    return q;
}

// ---- the combinations k_fuse_sum is instantiated for: every fuse layer of an HRNet (sources of shift s have C << s channels) and a
// lone source two levels down.  The one list: fuse_plan looks a call up here before it chooses a kernel, the dispatch of pam_fuse.hip
// instantiates row by row, and include/pam.h's "anything else: PAM_E_ARG" means this table.
struct FuseCombo { int C, n_up, sh[3]; };        // unused shifts are 0 (they are template arguments of the kernel)
constexpr FuseCombo FUSE_COMBOS[] = {
    {48, 1, {1, 0, 0}}, {48, 2, {1, 2, 0}}, {48, 3, {1, 2, 3}}, {96, 1, {1, 0, 0}}, {96, 2, {1, 2, 0}}, {96, 1, {2, 0, 0}}, {192, 1, {1, 0, 0}},
};
constexpr int FUSE_NCOMBO = sizeof(FUSE_COMBOS) / sizeof(FUSE_COMBOS[0]);

constexpr int fuse_combo(int C, int n_up, const int (&sh)[3]) {          // row of the table, -1: not instantiated
    for (int k = 0; k < FUSE_NCOMBO; ++k) {
        const FuseCombo& c = FUSE_COMBOS[k];
        bool same = c.C == C && c.n_up == n_up;
        for (int s = 0; s < 3 && same; ++s) same = s >= n_up || c.sh[s] == sh[s];
        if (same) return k;
    }
    return -1;
}

// rc: PAM_OK or PAM_E_ARG (nothing is launched).  kernel 1: the register-weights k_fuse_sum at anchor level L; 2: the persistent
// k_fuse_sum_lds.  The fields of the other kernel are 0.
struct FusePlan {
    int rc, kernel, combo;
    unsigned grid;
    // kernel 1: a unit = 2^ua_log x 2^ub_log anchor pixels (16 of them), units_y x units_x units per image, one workgroup per unit
    int L, ua_log, ub_log, units_y, units_x;
    // kernel 2: tiles of TA x TB pixels of the coarsest source, the LDS layout FLArgs carries, dynamic LDS bytes
    int TA, TB, tiles_y, tiles_x, ntiles;
    int w_off[3], w_bytes[3], bias_off, src_off[3], src_bytes, src_base, term_off[3];
    int lds_bytes;
};

inline FusePlan fuse_refused() { FusePlan p = {}; p.rc = PAM_E_ARG; return p; }

// ---- the argument check: everything the entry point refuses on integers alone (it checks the pointers itself)
inline bool fuse_args_ok(const FuseQuery& q) {
    const int C = q.C;
    if (q.N < 1 || q.H < 1 || q.W < 1 || (C != 48 && C != 96 && C != 192) || q.n_plain < 0 || q.n_plain > 2 || q.n_up < 1 || q.n_up > 3) return false;
    if ((size_t)q.N * q.H * q.W >= (1ull << 31)) return false;
    for (int t = 0; t < q.n_plain; ++t) {
        const int cs = q.plain_cs[t] > 0 ? q.plain_cs[t] : C;
        if (cs < C || cs % 8 != 0) return false;
    }
    int prev = 0;
    for (int s = 0; s < q.n_up; ++s) {
        const int sh = q.shift[s], cs = q.src_c[s];
        // sources in ascending shift (= branch) order; the map must be a whole number of source pixels (PyTorch's up-sampling needs that too)
        if (sh <= prev || sh > 5 || cs < 32 || cs % 32 != 0) return false;
        if (q.H % (1 << sh) != 0 || q.W % (1 << sh) != 0) return false;
        // the k loops are unrolled per (C, source channels): a source of shift s has C << s channels, as in every HRNet
        if (cs != C << sh) return false;
        prev = sh;
    }
    return true;
}

// ---- k_fuse_sum: the unit's rectangle of 16 anchor pixels at level L: the shape that covers the anchor map with the fewest units
// (ties: the squarest)
struct FuseUnits {
    int ua_log, ub_log, units_y, units_x;
    long long per_image() const { return (long long)units_y * units_x; }
};
inline FuseUnits fuse_units(int H, int W, int L) {
    const int HA = H >> L, WA = W >> L;
    const int shapes[5][2] = {{2, 2}, {1, 3}, {3, 1}, {0, 4}, {4, 0}};
    FuseUnits best = {};
    for (int k = 0; k < 5; ++k) {
        const FuseUnits u = {shapes[k][0], shapes[k][1], (HA + (1 << shapes[k][0]) - 1) >> shapes[k][0], (WA + (1 << shapes[k][1]) - 1) >> shapes[k][1]};
        if (k == 0 || u.per_image() < best.per_image()) best = u;
    }
    return best;
}

// ---- which kernel, which level.
// Which kernel (stand-alone times at 2 / 20 / 40 crops): the persistent LDS-weights form stays where it was not
// beaten.  C = 192 (12-wave workgroups, one per CU at a time): 18 units 8.2 us against its 7.7, 180 units 8.9 against 11.9, 360 units
// 16.9 against 16.8 -> register weights only for more than 64 units and no more than one per CU.  C = 96 under two sources: 540 units
// (level 1) 13.3 us against 14.3, 1 080 units 25.0 against 20.2 -> register weights up to 768 units.  The thresholds lie between the
// measured points; a caller that names a level (tile_a > 0) gets the register-weights kernel at any size.
// u1: the units of the whole call at level 1
constexpr bool fuse_takes_lds(int C, int n_up, int tile_a, long long u1, int n_cu) {
    return tile_a <= 0 && ((C == 192 && (u1 <= 64 || u1 > n_cu)) || (C == 96 && n_up == 2 && u1 > 768));
}
// k_fuse_sum_lds is instantiated for C = 96 and 192 only: no row of the table with another C may reach it at any size
constexpr bool fuse_lds_rows_are_96_192() {
    const long long sizes[5] = {1, 65, 256, 769, 1ll << 40};          // every side of every threshold
    for (int k = 0; k < FUSE_NCOMBO; ++k)
        for (int i = 0; i < 5; ++i)
            if (fuse_takes_lds(FUSE_COMBOS[k].C, FUSE_COMBOS[k].n_up, 0, sizes[i], 256) && FUSE_COMBOS[k].C != 96 && FUSE_COMBOS[k].C != 192) return false;
    return true;
}
static_assert(fuse_lds_rows_are_96_192(), "k_fuse_sum_lds<C> exists for C = 96, 192");

// the anchor level unless the caller names it: level 2 reads a wave's weights and the coarse sources' pixels a quarter as often, which
// pays from 18 k-steps of weights on (72 VGPRs) and only while there are units for half the CUs (level 1 below that: 4 times the
// workgroups).  A named level is clamped to 1 .. min(2, the coarsest shift).
inline int fuse_level(const FuseQuery& q, int smax, int ksteps) {
    int L = q.tile_a > 0 ? q.tile_a : ((smax >= 2 && ksteps >= 18 && q.N * fuse_units(q.H, q.W, 2).per_image() >= 128) ? 2 : 1);
    L = L > smax ? smax : L;
    return L > 2 ? 2 : L;
}

// ---- k_fuse_sum_lds: the LDS layout for a tile of TA x TB pixels of the coarsest source, written into p; false = does not fit (too
// many items per thread, a tile too tall or wide for the packed item index, or more LDS than a workgroup has)
inline bool fuse_lds_layout(const FuseQuery& q, int TA, int TB, FusePlan& p) {
    const int C = q.C, smax = q.shift[q.n_up - 1];
    if ((long)(TA << smax) * (TB << smax) * (C / 8) > 512L * FL_MAXI || (TA << smax) > 32767 || (TB << smax) > 255) return false;
    size_t o = 0;
    for (int s = 0; s < q.n_up; ++s) { p.w_off[s] = (int)o; p.w_bytes[s] = C * q.src_c[s] * 2; o += (size_t)p.w_bytes[s]; }
    p.bias_off = (int)o; o += (size_t)q.n_up * C * 4; o = (o + 1023) / 1024 * 1024;
    size_t sb = 0;
    for (int s = 0; s < q.n_up; ++s) { const int d = smax - q.shift[s]; p.src_off[s] = (int)sb; sb += (size_t)(TA << d) * (TB << d) * q.src_c[s] * 2; sb = (sb + 1023) / 1024 * 1024; }
    p.src_bytes = (int)sb; p.src_base = (int)o; o += 2 * sb;
    for (int s = 0; s < q.n_up; ++s) { const int d = smax - q.shift[s]; p.term_off[s] = (int)o; o += (size_t)(TA << d) * (TB << d) * C * 2; o = (o + 15) / 16 * 16; }
    p.TA = TA; p.TB = TB; p.lds_bytes = (int)o;
    return o <= (size_t)FL_LDS_MAX;
}

inline FusePlan fuse_plan_lds(const FuseQuery& q, int combo) {
    FusePlan p = {};
    p.kernel = 2; p.combo = combo;
    // the largest candidate that fits (FL_MAXI items per thread, LDS) and divides the coarsest map: an iteration costs two barriers and a
    // round of latencies whatever its size; a 16 x 24 tile of output 0 is 2 304 items.  No candidate divides the map: the largest that fits
    const int smax = q.shift[q.n_up - 1], Hc = q.H >> smax, Wc = q.W >> smax;
    const int cand[7][2] = {{8, 12}, {4, 6}, {4, 3}, {2, 3}, {1, 3}, {1, 2}, {1, 1}};
    bool found = false;
    for (int pass = 0; pass < 2 && !found; ++pass)
        for (int k = 0; k < 7 && !found; ++k)
            found = (pass == 1 || (Hc % cand[k][0] == 0 && Wc % cand[k][1] == 0)) && fuse_lds_layout(q, cand[k][0], cand[k][1], p);
    if (!found) return fuse_refused();
    const int OTH = p.TA << smax, OTW = p.TB << smax;
    p.tiles_y = (q.H + OTH - 1) / OTH; p.tiles_x = (q.W + OTW - 1) / OTW;
    const long long nt = (long long)q.N * p.tiles_y * p.tiles_x;
    if (nt >= (1ll << 30)) return fuse_refused();
    p.ntiles = (int)nt;
    // every workgroup walks the same number of tiles: 360 tiles -> 180 workgroups x 2 (not 256 of which 104 walk two); the CUs left over
    // take the other outputs' sums, which run on the branch streams at the same time
    int grid = q.max_workgroups > 0 && q.max_workgroups < q.n_cu ? q.max_workgroups : q.n_cu;
    const int per_wg = (p.ntiles + grid - 1) / grid;
    p.grid = (unsigned)((p.ntiles + per_wg - 1) / per_wg);
    return p;
}

// ---- the decision
inline FusePlan fuse_plan(const FuseQuery& q) {
    if (!fuse_args_ok(q)) return fuse_refused();
    const int combo = fuse_combo(q.C, q.n_up, q.shift);
    if (combo < 0) return fuse_refused();         // a combination no network here uses: not instantiated
    const int smax = q.shift[q.n_up - 1];
    int ksteps = 0;
    for (int s = 0; s < q.n_up; ++s) ksteps += q.src_c[s] / 32;
    if (fuse_takes_lds(q.C, q.n_up, q.tile_a, q.N * fuse_units(q.H, q.W, 1).per_image(), q.n_cu)) return fuse_plan_lds(q, combo);
    FusePlan p = {};
    p.kernel = 1; p.combo = combo; p.L = fuse_level(q, smax, ksteps);
    const FuseUnits u = fuse_units(q.H, q.W, p.L);
    const long long nu = q.N * u.per_image();
    if (nu >= (1ll << 31)) return fuse_refused();
    p.ua_log = u.ua_log; p.ub_log = u.ub_log; p.units_y = u.units_y; p.units_x = u.units_x; p.grid = (unsigned)nu;
    return p;
}

// what pam_fuse_sum_plan writes: {kernel, L (0 for kernel 2), unit rows log2 | TA, unit columns log2 | TB, units_y | tiles_y,
// units_x | tiles_x, grid, dynamic LDS bytes}
inline void fuse_plan_out8(const FusePlan& p, int32_t* out8) {
    const bool reg = p.kernel == 1;
    const int32_t o[8] = {p.kernel, p.L, reg ? p.ua_log : p.TA, reg ? p.ub_log : p.TB, reg ? p.units_y : p.tiles_y, reg ? p.units_x : p.tiles_x,
                          (int32_t)p.grid, p.lds_bytes};
    for (int k = 0; k < 8; ++k) out8[k] = o[k];
}
