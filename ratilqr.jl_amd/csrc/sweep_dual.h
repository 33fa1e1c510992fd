// sweep_dual.h -- TWO independent Riccati recursions per wavefront over ONE pass through a trajectory's tiles.
//
//   recursion A : policy evaluation            solve_approximate_dp   (ileqg.jl:412-465)
//                   mode 6: initialize!'s open-loop sweep (L = 0, mu = 0)          (ileqg.jl:234)
//                   mode 7: line-search candidate 0 under the current gains         (ileqg.jl:522-528)
//   recursion B : the gain sweep the NEXT step! will run on these very tiles        solve_approximate_dp!  (ileqg.jl:341-406)
//                   (step! re-linearises the accepted trajectory, App. B.1: if candidate 0 is accepted -- or, in mode 6, if
//                   initialize! succeeds -- B's gains, mu, Delta are exactly what the reference computes next; otherwise they are
//                   discarded by ls_select_kernel / commit_init_kernel).  Its output goes to the idle half of the gain buffers.
//
// Why: at E = 1 a sweep kernel runs one wave per SIMD and that wave is idle ~45 % of its cycles waiting on its own serial
// pivot chain (profiles/r01_pmc_sq_E1.md).  Two waves per SIMD overlapped poorly; two recursions inside ONE wave give the
// compiler two independent dependency chains to interleave in a single basic block, and the tiles are read once for both.
// Every arithmetic expression is the one of sweep_kernel, so results are bit-identical to the unfused order (tested).
//
// B has no mu-restart loop here: if H is not PD (or M is not PD) B is abandoned (spec_st = 0 / 2) and A continues; the plain
// gain sweep then runs for that sample in the next round, restarts included.
#pragma once
#include "device_utils.h"
#include "kernels.h"
#include "layout.h"

// FLY sweeps (policy evaluation of the speculative path's line-search candidates, LQ family): the record of a candidate holds only its
// [c_x | c_u | c] row (rollin_body<.., NOTILE>); f_x | f_u and the cost Hessian of step t are formed here from x_t and the problem tables --
// the expressions of the rollout kernels' tile stores, so the registers hold the bits a materialised record would have delivered.
// FLY: 0 records are complete, 1 time-invariant cost tables (register images, loaded once), 2 time-varying cost tables (loaded per step)
struct FlyCtx {
    double zt[3], dg[3];   // register image of [A | B]; 1 on the lane that holds the diagonal element of f_x in that register
    d4 cc;                 // register image of [[Q, 0], [P, R]] (FLY == 1)
    double mq, kappa;
    const double *xh;      // state history of the trajectory
    const double *ctab;    // FLY == 2
};
__device__ __forceinline__ void fly_init(FlyCtx &fc, const ProblemDev &pb, const double *xh, int l, int g, int j, bool tv) {
    fc.mq = (j < 12) ? 1.0 : 0.0;
    fc.kappa = pb.kappa;
    fc.xh = xh;
    fc.ctab = pb.Ctab;
#pragma unroll
    for (int r = 0; r < 3; ++r) { fc.zt[r] = pb.Zt[64 * r + l]; fc.dg[r] = (j == 4 * r + g) ? 1.0 : 0.0; }
    fc.cc = (d4){0, 0, 0, 0};
    if (!tv) {
#pragma unroll
        for (int r = 0; r < 3; ++r) fc.cc[r] = pb.Ctab[64 * r + l] * fc.mq;
        fc.cc[3] = pb.Ctab[192 + l];
    }
}

struct DTile {
    d4 z, c;
    double x, la;          // x: lanes 0..15 = qr, lane 16 = q (register-image record, layout.h); la: own entry L[g][j] of the gain row block
    double xj;             // FLY: x_t[j] of this lane's column
};

// End of a recording gain pass (SweepArgs.rec, one lane): the record becomes the sample's valid one under a new generation -- which the gains the
// pass wrote to L / dl half `half` carry -- or, if the pass failed or met a non-finite value (bad), no record is valid and that half carries none.
__device__ __forceinline__ void rec_close(const RecDev &rc, const int b, const int half, const bool bad, const double mu, const double rprod, const int rexp) {
    const int g0 = rc.gen[b], gabs = g0 < 0 ? -g0 : g0, gnew = gabs + 1;
    if (bad) {
        rc.gen[b] = -gabs;
        rc.lgen[2 * b + half] = 0;
    } else {
        rc.gen[b] = gnew;
        rc.mu[b] = mu;
        rc.rprod[b] = rprod;
        rc.rexp[b] = rexp;
        rc.lgen[2 * b + half] = gnew;
    }
}

// HASL: recursion A evaluates a given policy (mode 7); false for initialize!'s open-loop sweep (mode 6: all gains zero, nothing to load)
template <bool HASL, int FLY = 0>
__device__ __forceinline__ void dload(DTile &tr, const double *__restrict__ tp, int lx, int l, int j,
                                      const double *__restrict__ Lp, double mL, int g, const FlyCtx *fc = nullptr, int t = 0) {
    if (FLY) {
        tr.xj = fc->xh[(long)t * XSTR + ((j < 12) ? j : 11)];
        if (FLY == 2) {
            const double *__restrict__ C = fc->ctab + (long)t * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) tr.c[r] = C[64 * r + l];
        }
    } else {
        const double2 *__restrict__ t2 = reinterpret_cast<const double2 *>(tp);
        const int c34 = TS_REG(3, l), r5 = TS_REG(5, l);            // (loop-invariant per lane; dead lanes: the record's zero pair)
        const double2 w0 = t2[l], w1 = t2[64 + l], w2 = *reinterpret_cast<const double2 *>(tp + c34);
        tr.z[0] = w0.x; tr.z[1] = w0.y; tr.z[2] = w1.x; tr.z[3] = 0.0;
        tr.c[0] = w2.x; tr.c[1] = w2.y; tr.c[2] = tp[r5];
        tr.c[3] = w1.y;
    }
    tr.x = tp[TS_QR + lx];
    const int jc = (j < 12) ? j : 11;
    tr.la = HASL ? Lp[g * 12 + jc] * mL : 0.0;
}

// The elimination rounds of the two recursions are the shared elim_round (device_utils.h: rank-2 update on the matrix pipe, no LDS,
// no fence), issued back to back: two independent pivot chains for the scheduler to interleave.
// wls: this wavefront's LDS scratch (WLS_DUAL doubles)
// REC (solve_fused_kernel<.., RPL>): recursion B writes the Riccati-matrix record of its steps (see sweep_body)
template <int WM, bool HASL, int FLY = 0, bool REC = false>
__device__ __forceinline__ void sweep_dual_body(const SweepArgs &a, const int b, double *const wls) {
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));      // opaque per phase (see sweep_body)
    const int l_ = lane_, g_ = l_ >> 4, j_ = l_ & 15;
    const int l = l_, g = g_, j = j_;
    const StateDev &st = a.st;
    const ProblemDev &pb = a.pb;
    [[maybe_unused]] const int dgs = 20 + 4 * (a.mode - 6);
    BODY_MARK(a.dump, dgs + 0);
    // (per-sample scalars fetched before the first test on any of them: see sweep_body)
    int slot, cidx = -1;
    const int v_act = st.ls_active[b], v_flag = st.flag_c[b * st.E], v_nom = st.slot_nom[b], v_stat = st.status[b], v_sel = st.lsel[b];
    const int s_act = wave_uniform(v_act), s_flag = wave_uniform(v_flag), s_nom = wave_uniform(v_nom), s_stat = wave_uniform(v_stat), sel = wave_uniform(v_sel);
    const double theta = st.theta[b], muB = st.mu[b];          // initialize! leaves mu = 0 (set by init_state_kernel)
    if (a.mode == 7) {
        if (!s_act) return;
        cidx = b * st.E;
        if (s_flag == 2) return;
        slot = cand_slot(b, 0, s_nom, st.E);
    } else {
        if (s_stat != ST_RUNNING) return;
        slot = b * (st.E + 1) + s_nom;
    }
    const double muA = (a.mode == 6) ? 0.0 : muB;
    const int N = st.N;
    if (a.mode == 7) BODY_MARK(a.dump, 28);
    const double *__restrict__ tile0 = st.tiles + tile_slot(st, b, slot) * st.tile_stride;
    FlyCtx fc;
    if (FLY) fly_init(fc, pb, st.xs + (long)slot * st.x_stride, l, g, j, FLY == 2);
    const double *__restrict__ Lb = st.L + (long)sel * st.l_half + (long)b * N * LSTR;
    double *__restrict__ Lout = st.L + (long)(sel ^ 1) * st.l_half + (long)b * N * LSTR;
    double *__restrict__ dlout = st.dl + (long)(sel ^ 1) * st.dl_half + (long)b * N * USTR;

    double *const lbufA = wls;
    double *const exA = wls + 64, *const exB = wls + 64 + 168;         // [G|H] 4x16, f 16, [80] = 0, [84..99] = s_vec, [104..] dump slots
                                                                       // of the idle lanes (unconditional writes: see sweep_body)
    if (l < 8) { exA[80 + l] = 0.0; exB[80 + l] = 0.0; }

    const double mL = (a.mode == 7 && j < 12) ? 1.0 : 0.0;
    const double m12 = (j < 12) ? 1.0 : 0.0;
    const double nth12 = -theta * m12;
    const double mA_ = (g == 0 && j < 12) ? 1.0 : 0.0, mB_ = (g == 0 && j == 12) ? 1.0 : 0.0, mH = (j == 12 + g) ? 1.0 : 0.0;
    ElimMasks em;
    elim_masks(em, g, j);
    int hoff[4], foff[3], goff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hoff[k] = (g <= k) ? (g * 16 + 12 + k) : (k * 16 + 12 + g);
        goff[k] = (j < 12) ? (k * 16 + j) : (j == 12 ? 64 + 12 + k : 80);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) foff[r] = (j == 12) ? (64 + 4 * r + g) : 80;
    const int gaoff = (j == 12) ? (64 + 12 + g) : 80;
    const int lx = (l < 17) ? l : TS_PAD - TS_QR;
    const int svo = (g == 0) ? 84 + j : 104 + l, fbo = (g == 0) ? 64 + j : 104 + l;
    double *const pgl = (j < 12) ? Lout + g * 12 + j : (j == 12 ? dlout + g : sample_sink(st, b) + l);
    const long sgl = (j < 12) ? LSTR : (j == 12 ? USTR : 0);

    d4 winv = {0, 0, 0, 0}, wp = {0, 0, 0, 0};
    double epall = 1.0;
    double nwrow[3] = {0.0, 0.0, 0.0};                           // WM == 2 (W diagonal): see sweep_body
    if (WM == 2) {
#pragma unroll
        for (int r = 0; r < 3; ++r) nwrow[r] = -pb.Wdg[4 * r + g];
    }
    if (WM != 1) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { winv[r] = pb.Winv[64 * r + l]; wp[r] = pb.Wp[64 * r + l]; }
        epall = ((((pb.epiv[0] * pb.epiv[2]) * pb.epiv[4]) * pb.epiv[6]) * pb.epiv[8]) * pb.epiv[10];
    }
    const double coef = (theta != 0.0) ? -1.0 / (2.0 * theta) : 0.0;

    // terminal condition (ileqg.jl:352-354 / 429-431): both recursions start from the same V_N
    d4 vA, vB;
    {
        const double *__restrict__ tt = tile0 + (long)N * TSTRIDE;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = 4 * r + g;
            // (one unconditional load per register, the address selected per lane: conditional loads compile to a chain of divergent
            //  branches, each waiting for its own round trip -- 4.3 k cycles of prologue measured in the fused kernel)
            const double te = tt[(j < 12) ? TT_Q + i * 12 + j : TT_QV + i];
            vA[r] = (j <= 12) ? te : 0.0;
        }
        const double t3 = tt[(j < 12) ? TT_QV + j : TT_q];
        vA[3] = (g == 0 && j <= 12) ? (j < 12 ? t3 : 2.0 * t3) : 0.0;
        vB = vA;
    }
#ifdef RAT_DIAG_PHASES
    if (a.mode == 7) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); BODY_MARK(a.dump, 29); }
#endif
    double raccA = 0.0, raccB = 0.0, rprodA = 1.0, rprodB = 1.0;
    int rexpA = 0, rexpB = 0;
    int failA = 0, deadB = 0;        // deadB: 1 = H not PD (needs the restart loop of the plain kernel), 2 = M not PD
    [[maybe_unused]] double *const recp = REC ? a.rec.m + (long)b * N * REC_STEP + 4 * l : nullptr;
    [[maybe_unused]] double rchk = 0.0;                           // REC: stays zero while every recorded value is finite

    DIAG_DECL
    auto step = [&](const int t, const DTile &cur) -> int {
        int l = l_, g = g_, j = j_;
        asm volatile("" : "+v"(l), "+v"(g), "+v"(j));
        DIAG_START();
        if (WM == 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { winv[r] = pb.Winv[(long)t * 192 + 64 * r + l]; wp[r] = pb.Wp[(long)t * 192 + 64 * r + l]; }
            { const double *ept = pb.epiv + (long)t * 16; epall = ((((ept[0] * ept[2]) * ept[4]) * ept[6]) * ept[8]) * ept[10]; }
        }
        d4 cz, ccs;                                                  // the step's tile: from the record, or (FLY) formed here (see FlyCtx)
        if (!FLY) { cz = cur.z; ccs = cur.c; }
        else {
#pragma unroll
            for (int r = 0; r < 3; ++r) cz[r] = fx_diag(fc.zt[r], fc.dg[r], fc.kappa, cur.xj);
            cz[3] = 0.0;
            if (FLY == 2) { ccs[0] = cur.c[0] * fc.mq; ccs[1] = cur.c[1] * fc.mq; ccs[2] = cur.c[2] * fc.mq; ccs[3] = cur.c[3]; }
            else ccs = fc.cc;
        }
        d4 xzA, xzB;                                                 // (WM == 2: formed inside the theta == 0 branch, see sweep_body)
        if (WM != 2) {
            xzA = mm3(vA, cz, (d4){0, 0, 0, 0});
            xzB = mm3(vB, cz, (d4){0, 0, 0, 0});
        }
        d4 tmA, tmB;
        [[maybe_unused]] double mrec[3] = {0.0, 0.0, 0.0};          // REC: -M^-1 of recursion B as recorded (theta == 0: no valid record)
        if (theta != 0.0) {
            exA[svo] = vA[3]; exB[svo] = vB[3];
            d4 mA, mB;
#pragma unroll
            for (int r = 0; r < 3; ++r) { mA[r] = fma(nth12, vA[r], winv[r]); mB[r] = fma(nth12, vB[r], winv[r]); }
            mA[3] = 0.0; mB[3] = 0.0;
            int pdA = 1, pdB = 1;
            rprodA *= epall; rprodB *= epall;
            DIAG_STAMP(0, mA[0]);
            elim_round_pair<0>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            elim_round_pair<1>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            elim_round_pair<2>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            elim_round_pair<3>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            elim_round_pair<4>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            elim_round_pair<5>(mA, mB, em, pdA, pdB, rprodA, rprodB);
            DIAG_STAMP(1, mA[0]);
            if (!(pdA > 0) || !(rprodA * 0.0 == 0.0)) { failA = 1; return 1; }    // @assert isposdef(M) (:440)
            if (!deadB && (!(pdB > 0) || !(rprodB * 0.0 == 0.0))) deadB = 2;      // @assert isposdef(M) (:366)
            rexpA += __builtin_amdgcn_frexp_exp(rprodA); rprodA = __builtin_amdgcn_frexp_mant(rprodA);
            rexpB += __builtin_amdgcn_frexp_exp(rprodB); rprodB = __builtin_amdgcn_frexp_mant(rprodB);
            if (REC) {                                               // (stored below, once the step's factor of H can ride along)
                mrec[0] = mB[0]; mrec[1] = mB[1]; mrec[2] = mB[2];
            }
            if (WM == 2) {
                raccA = racc_diag(raccA, nth12, exA[84 + j], mA[0], mA[1], mA[2], exA[84 + g], exA[84 + 4 + g], exA[84 + 8 + g]);
                raccB = racc_diag(raccB, nth12, exB[84 + j], mB[0], mB[1], mB[2], exB[84 + g], exB[84 + 4 + g], exB[84 + 8 + g]);
                d4 mwA, mwB;
#pragma unroll
                for (int r = 0; r < 3; ++r) { mwA[r] = mA[r] * nwrow[r]; mwB[r] = mB[r] * nwrow[r]; }
                mwA[3] = 0.0; mwB[3] = 0.0;
                const d4 y2A = mm3(mwA, cz, (d4){0, 0, 0, 0});
                const d4 y2B = mm3(mwB, cz, (d4){0, 0, 0, 0});
                tmA = mm3(vA, y2A, (d4){0, 0, 0, 0});
                tmB = mm3(vB, y2B, (d4){0, 0, 0, 0});
            } else {
                d4 minvA, minvB;
#pragma unroll
                for (int r = 0; r < 3; ++r) { minvA[r] = nth12 * mA[r]; minvB[r] = nth12 * mB[r]; }
                minvA[3] = 0.0; minvB[3] = 0.0;
                raccA += exA[84 + j] * (minvA[0] * exA[84 + g] + minvA[1] * exA[84 + 4 + g] + minvA[2] * exA[84 + 8 + g]);
                raccB += exB[84 + j] * (minvB[0] * exB[84 + g] + minvB[1] * exB[84 + 4 + g] + minvB[2] * exB[84 + 8 + g]);
                const d4 y2A = mm3(minvA, xzA, (d4){0, 0, 0, 0});
                const d4 y2B = mm3(minvB, xzB, (d4){0, 0, 0, 0});
                tmA = mm3(vA, y2A, xzA);
                tmB = mm3(vB, y2B, xzB);
            }
        } else {
            // theta == 0: the reference still asserts isposdef(inv(W) - 0 S) (:365-366 / :439-440): a non-finite S fails it
            const double nfA = fma(vA[2], 0.0, fma(vA[1], 0.0, vA[0] * 0.0)), nfB = fma(vB[2], 0.0, fma(vB[1], 0.0, vB[0] * 0.0));
            if (__ballot(nfA != nfA) & 0x0FFF0FFF0FFF0FFFull) { failA = 1; return 1; }
            if (!deadB && (__ballot(nfB != nfB) & 0x0FFF0FFF0FFF0FFFull)) deadB = 2;
            raccA = fma(m12, fma(wp[2], vA[2], fma(wp[1], vA[1], wp[0] * vA[0])), raccA);
            raccB = fma(m12, fma(wp[2], vB[2], fma(wp[1], vB[1], wp[0] * vB[0])), raccB);
            if (WM == 2) { tmA = mm3(vA, cz, (d4){0, 0, 0, 0}); tmB = mm3(vB, cz, (d4){0, 0, 0, 0}); }
            else { tmA = xzA; tmB = xzB; }
        }
        DIAG_STAMP(2, tmA[0]);
        d4 fA = mm3(cz, tmA, ccs);
        d4 fB = mm3(cz, tmB, ccs);
        const double ghA = fma(muA, mH, fA[3]), ghB = fma(muB, mH, fB[3]);
        if (REC) {
            recp[(long)t * REC_STEP + 3] = ghB;
            rchk = fma(ghB, 0.0, rchk);
        }
        const double fvA = tmA[3] + cur.x, fvB = tmB[3] + cur.x;
        exA[g * 16 + j] = ghA; exB[g * 16 + j] = ghB;
        exA[fbo] = fvA; exB[fbo] = fvB;
        if (HASL) lbufA[l] = cur.la;                            // rows of [L | dl] of the given policy to every lane
        DIAG_STAMP(3, ghB);
        WAVE_SYNC();
        // ---- A: given policy (:446-451) ----
        const double hA0 = exA[hoff[0]], hA1 = exA[hoff[1]], hA2 = exA[hoff[2]], hA3 = exA[hoff[3]];
        const double gaA = fma(ghA, m12, exA[gaoff]);
        const double uaA = HASL ? ua_entry(hA0, hA1, hA2, hA3, lbufA[j], lbufA[16 + j], lbufA[32 + j], lbufA[48 + j], gaA) : gaA;
        // ---- B: optimal gains (:372-382) ----
        const double hB0 = exB[hoff[0]], hB1 = exB[hoff[1]], hB2 = exB[hoff[2]], hB3 = exB[hoff[3]];
        const double gaB = fma(ghB, m12, exB[gaoff]);
        const double h00 = exB[12], h01 = exB[13], h02 = exB[14], h03 = exB[15];
        const double h11 = exB[16 + 13], h12 = exB[16 + 14], h13 = exB[16 + 15];
        const double h22 = exB[32 + 14], h23 = exB[32 + 15], h33 = exB[48 + 15];
        const double g0 = exB[goff[0]], g1 = exB[goff[1]], g2 = exB[goff[2]], g3 = exB[goff[3]];
        const Ldl4 f = ldl4_factor(h00, h01, h02, h03, h11, h12, h13, h22, h23, h33);
        const double l10 = f.l10, l20 = f.l20, l30 = f.l30, l21 = f.l21, l31 = f.l31, l32 = f.l32, i0 = f.i0, i1 = f.i1, i2 = f.i2, i3 = f.i3;
        if (!deadB && !(h00 > 0.0 && f.d1 > 0.0 && f.d2 > 0.0 && f.d3 > 0.0)) deadB = 1;    // !isposdef(H) (:372): left to the plain kernel
        if (REC) {
            // the record's -M^-1 words, the factor on the lanes of column 12 (layout.h: REC_FACT_*; nothing in this pass reads mrec again).
            // Every value is on every lane: a per-lane select, exact for any bits; a non-finite one invalidates the record through rchk
            const double fv[12] = {f.l10, f.l20, f.l30, f.l21, f.l31, f.l32, f.d1, f.d2, f.i0, f.i1, f.i2, f.i3};
            const bool g1 = g & 1, g2 = g & 2, fl = (j == REC_FACT_J);
            double w[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double lo = g1 ? fv[REC_FACT_VAL(1, r)] : fv[REC_FACT_VAL(0, r)], hi = g1 ? fv[REC_FACT_VAL(3, r)] : fv[REC_FACT_VAL(2, r)];
                w[r] = fl ? (g2 ? hi : lo) : mrec[r];
            }
            *reinterpret_cast<double2 *>(recp + (long)t * REC_STEP) = make_double2(w[0], w[1]);
            recp[(long)t * REC_STEP + 2] = w[2];
            rchk = fma((w[0] + w[1]) + w[2], 0.0, rchk);
        }
        const double y0 = -g0;
        const double y1 = -g1 - l10 * y0;
        const double y2 = -g2 - l20 * y0 - l21 * y1;
        const double y3 = -g3 - l30 * y0 - l31 * y1 - l32 * y2;
        const double x3 = y3 * i3;
        const double x2 = y2 * i2 - l32 * x3;
        const double x1 = y1 * i1 - l21 * x2 - l31 * x3;
        const double x0 = y0 * i0 - l10 * x1 - l20 * x2 - l30 * x3;
        const double laB = ((x0 * em.e0[0] + x1 * em.e1[0]) + x2 * em.e0[1]) + x3 * em.e1[1];     // row g takes x_g (see sweep_body)
        const double uaB = ua_entry(hB0, hB1, hB2, hB3, x0, x1, x2, x3, gaB);
        pgl[(long)t * sgl] = (j <= 12) ? laB : 0.0;                // L_t | dl_t | idle lanes: sink
        d4 fxA, fxB;
#pragma unroll
        for (int r = 0; r < 3; ++r) { fxA[r] = fma(fA[r], m12, exA[foff[r]]); fxB[r] = fma(fB[r], m12, exB[foff[r]]); }
        const double qc = readlane_f64(cur.x, 16);
        fxA[3] = fma(fvA, mA_, (2.0 * qc + vA[3]) * mB_);
        fxB[3] = fma(fvB, mA_, (2.0 * qc + vB[3]) * mB_);
        DIAG_STAMP(4, uaB);
        d4 vnB = MFMA(laB, uaB, fxB);
        vnB = MFMA(gaB, laB, vnB);
        if (HASL) {
            d4 vnA = MFMA(cur.la, uaA, fxA);
            vA = MFMA(gaA, cur.la, vnA);
        } else {
            vA = fxA;                                           // zero gains: V = Fx
        }
        vB = vnB;
        DIAG_STAMP(5, vB[0]);
        WAVE_SYNC();
        return 0;
    };

    if (a.mode == 7) BODY_MARK(a.dump, 30);
    DTile ra, rb2;
    dload<HASL, FLY>(ra, tile0 + (long)(N - 1) * TSTRIDE, lx, l, j, Lb + (long)(N - 1) * LSTR, mL, g, &fc, N - 1);
    BODY_MARK(a.dump, dgs + 1);
    for (int t = N - 1; t >= 0; t -= 2) {
        {
            const int tn = (t > 0) ? t - 1 : 0;
            dload<HASL, FLY>(rb2, tile0 + (long)tn * TSTRIDE, lx, l, j, Lb + (long)tn * LSTR, mL, g, &fc, tn);
        }
        if (step(t, ra)) break;
        if (t == 0) break;
        {
            const int tn = (t > 1) ? t - 2 : 0;
            dload<HASL, FLY>(ra, tile0 + (long)tn * TSTRIDE, lx, l, j, Lb + (long)tn * LSTR, mL, g, &fc, tn);
        }
        if (step(t - 1, rb2)) break;
    }
    BODY_MARK(a.dump, dgs + 2);
#ifdef RAT_DIAG
    if (l_ == 0 && blockIdx.x < 8 && a.dump)
        for (int q = 0; q < 6; ++q) a.dump[128 + blockIdx.x * 8 + q] = (double)dg_acc[q];
#endif
    const double totA = sweep_scalars(wave_sum(raccA), coef, rprodA, rexpA, theta != 0.0);
    (void)raccB; (void)rprodB; (void)rexpB;          // B's value s_1 is not used by step! (only L, dl, mu, Delta are)
    if (REC) {            // B ran every step (A did not fail), solved them all, on finite data, with theta != 0: its record is valid
        const bool bad = failA || deadB || theta == 0.0 || __ballot(!(rchk == 0.0));
        if (l == 12) rec_close(a.rec, b, sel ^ 1, bad, muB, rprodB, rexpB);
    }
    if (l == 12) {
        const double s0 = 0.5 * vA[3] + totA;
        if (a.mode == 7) {
            st.value_c[cidx] = s0;
            st.flag_c[cidx] = failA ? 1 : 0;
            if (a.prune) {
                // Will line_search! settle on this candidate (ileqg.jl:538, or the forced accept of :557-558)?  Then the sequential rule never
                // reads candidates 1 .. E-1 of this round: their evaluation waves poll this word and stop (sweep_body<.., PRUNE>).
                const double cur = st.value[b], eps = st.ls_eps[b];
                const bool take = !failA && (isapprox_default(s0, cur) || s0 < cur || eps * a.op.lambda < a.op.eps_min);
                __atomic_store_n(&st.acc0[b], take ? 1 : 0, __ATOMIC_RELAXED);
            }
        } else {
            st.value[b] = failA ? INFINITY : s0;
            if (failA) st.status[b] = 1;                      // RAT_ST_M_NOT_PD_INIT
        }
        st.mu_spec[b] = muB;                                   // no restart happened: mu, Delta unchanged by the gain sweep
        st.delta_spec[b] = st.delta[b];
        st.spec_st[b] = (failA || deadB == 1) ? 0 : (deadB == 2 ? 2 : 1);
    }
    BODY_MARK(a.dump, dgs + 3);
}


// =======================================================================================================================================
// replay_body: a sweep of the one-wavefront-per-sample solve running only the VECTOR half of its recursions over ONE stream: the record of the
// sample's last full paired gain sweep (SweepArgs.rec).
//   GAINB = true   replay_dual_body: mode 7 of sweep_dual_body -- line-search candidate 0's evaluation and the gain sweep of the next step!
//   GAINB = false  replay_eval_body: mode 1 of sweep_body -- the plain evaluation of candidate 0 where accepting it ends the solve (d < d_tol
//                  or iter_max: nothing would consume the gains), the evaluation half of the pair alone
// Why it is exact: for the LQ family with kappa = 0 and a time-invariant diagonal W, f_x | f_u and the cost Hessian do not depend on the
// trajectory, so S_t, -M_t^-1, [G_t | H_t + mu I] and L_t of a sweep depend only on theta and mu -- and the evaluation of the L a gain sweep
// produced forms S = Q + A'DSA + L'HL + L'G + G'L from the same operands as that sweep (sweep_body: one formula for both, Ua in one rounding
// order everywhere: ua_entry).  The matrix half of the V update only feeds the matrix half (an MFMA element reads its own row of A and column
// of B; F reads rows 0..11 of T), so what the vector half reads from it -- -M^-1 (racc and Y = -M^-1 (-inv W) [A|B]) and register 3 of
// F + mu I -- is taken from the record, and every value that reaches an output or feeds back comes from the instruction and the operands of
// the full sweep:
//   T row 12 = mm3(v, Y) (rows 0..11 of the result are not used), the theta s'M^-1 s term (racc_diag), [G | g], the LDL' of H and the solve
//   of every column (the columns j < 12 give L_t again: a replayed gain sweep writes L_t and dl_t like a full one), Ua, and the two V-update
//   MFMAs (row 12 and column 12 of V are two differently rounded copies of s_vec; both feed forward).  The S block of V is not formed (Fx's is 0).
// Exactness needs finite vector data: a non-finite x_t^2 (kappa = 0 still forms 0 x^2) or s_vec gives NaNs the record does not have.  Every
// step tests its operands first; on one the replay stops (before the step's stores) and returns false -- so does a sweep the gate refuses
// (no valid record, mu differs bitwise from the recorded pass's, theta == 0, or committed gains not solved from this record; the evaluation
// alone also under rec.last = 0) -- and the caller runs the full sweep, which rewrites everything the replay wrote.  Record loads run two steps
// ahead (three register sets).
// STACK (GAINB only; switch lq_replay_stack): row 12 of T for BOTH recursions from one mm3.  mm3(v, Y) is v'Y: row i of the result reads
// column i of v (registers 0..2 on the lanes j == i) and nothing else of it, and only row 12 of T is used -- so columns 0..11 of the operand
// are free.  Column 12 of recursion B's V is rotated into column 4 of a copy of recursion A's (one DPP row rotation by eight with a bank
// mask: columns 4..7 <- B's 12..15, the rest A's own), one mm3 runs against Y, and row 12 (register 3, g == 0) is recursion A's T row,
// row 4 (register 1, g == 0) recursion B's: the same column of V, the same Y, the same K order and start value as the two separate
// mm3 -- the same bits, on the lanes that read them before.  13 MFMAs per step become 10.
// FACT (GAINB only; switch lq_replay_factor): the LDL' of H is not formed again.  H + mu I is matrix data: the factor every lane would compute
// from the recorded H is the one recursion B of the recording pass computed at that step (one helper, one rounding order: ldl4_factor), and
// that pass stored it on the column-12 lanes of the three -M^-1 words (layout.h: REC_FACT_*).  Those lanes copy their words to twelve idle
// doubles of exB before the step's fence, every lane reads the ten values the substitutions need; the substitutions, laB, Ua and the
// V update are the same source either way.
// wls: WLS_DUAL doubles
// =======================================================================================================================================
struct RTile {
    double2 m01, m2h;      // record: -M^-1 registers 0, 1 | register 2, [G | H + mu I]
    double x, xj, la;      // [qr | q] row, x_t[j], own entry of L_t (evaluation)
};

template <bool GAINB, bool STACK = false, bool FACT = false>
__device__ __forceinline__ bool replay_body(const SweepArgs &a, const int b, double *const wls) {
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));      // opaque per phase (see sweep_body)
    const int l_ = lane_, g_ = l_ >> 4, j_ = l_ & 15;
    const int l = l_, g = g_, j = j_;
    const StateDev &st = a.st;
    const ProblemDev &pb = a.pb;
    const RecDev &rc = a.rec;
    // (every per-sample word requested before the first test on any of them: see sweep_body)
    const int v_act = st.ls_active[b], v_flag = st.flag_c[b * st.E], v_nom = st.slot_nom[b], v_sel = st.lsel[b];
    const int v_gen = rc.gen[b], v_lg0 = rc.lgen[2 * b], v_lg1 = rc.lgen[2 * b + 1];
    const double v_theta = st.theta[b], v_mu = st.mu[b], v_rmu = rc.mu[b], v_rprod = rc.rprod[b];
    const int v_rexp = rc.rexp[b];
    const int s_act = wave_uniform(v_act), s_flag = wave_uniform(v_flag), s_nom = wave_uniform(v_nom), sel = wave_uniform(v_sel);
    const int gen = wave_uniform(v_gen), lg = wave_uniform(sel ? v_lg1 : v_lg0);
    const double theta = readlane_f64(v_theta, 0), mu = readlane_f64(v_mu, 0), rmu = readlane_f64(v_rmu, 0);
    if (!s_act || s_flag == 2 || a.prune) return false;
    if (!GAINB && !rc.last) return false;                        // switch lq_replay_last
    // (mu = 0 only: with a raised mu the replayed pair was measured to differ from the full one in the last bits of some line-search
    //  candidates' values -- not explained yet -- while every pair at mu = 0 matched; the LQ family raises mu only where H is not PD)
    if (gen <= 0 || lg != gen || theta == 0.0 || __double_as_longlong(mu) != 0 || __double_as_longlong(rmu) != 0) return false;
    const int slot = cand_slot(b, 0, s_nom, st.E);
    const int N = st.N;
    const double *__restrict__ tile0 = st.tiles + tile_slot(st, b, slot) * st.tile_stride;
    const double *__restrict__ xh = st.xs + (long)slot * st.x_stride;
    const double *__restrict__ rp = rc.m + (long)b * N * REC_STEP + 4 * l;
    const int osel = sel ^ 1;
    const double *__restrict__ Lb = st.L + (long)sel * st.l_half + (long)b * N * LSTR;
    double *__restrict__ Lout = st.L + (long)osel * st.l_half + (long)b * N * LSTR;
    double *__restrict__ dlout = st.dl + (long)osel * st.dl_half + (long)b * N * USTR;

    double *const lbuf = wls;                                    // evaluation: the step's gain rows [L | 0] (natural 4 x 16 layout)
    double *const exA = wls + 64, *const exB = wls + 64 + 168;   // exchange areas (see sweep_body); [G | H] lives in exB
    if (l < 8) { exA[80 + l] = 0.0; exB[80 + l] = 0.0; }

    const double m12 = (j < 12) ? 1.0 : 0.0;                    // (also the gain-column multiplier of the evaluation's loads)
    const double nth12 = -theta * m12;
    const double mA_ = (g == 0 && j < 12) ? 1.0 : 0.0, mB_ = (g == 0 && j == 12) ? 1.0 : 0.0;
    [[maybe_unused]] const double e00 = (g == 0) ? 1.0 : 0.0, e10 = (g == 1) ? 1.0 : 0.0, e01 = (g == 2) ? 1.0 : 0.0, e11 = (g == 3) ? 1.0 : 0.0;
    int hoff[4], foff[3];
    [[maybe_unused]] int goff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hoff[k] = (g <= k) ? (g * 16 + 12 + k) : (k * 16 + 12 + g);
        goff[k] = (j < 12) ? (k * 16 + j) : (j == 12 ? 64 + 12 + k : 80);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) foff[r] = (j == 12) ? (64 + 4 * r + g) : 80;
    const int gaoff = (j == 12) ? (64 + 12 + g) : 80;
    const int lx = (l < 17) ? l : TS_PAD - TS_QR;
    const int jc = (j < 12) ? j : 11;
    const int svo = (g == 0) ? 84 + j : 104 + l, fbo = (g == 0) ? 64 + j : 104 + l;
    [[maybe_unused]] const int fwo = (j == REC_FACT_J) ? EX_FACT + REC_FACT_VAL(g, 0) : EX_FACT_SINK;     // FACT: where this lane's three words go
    const int sro = (j == REC_FACT_J) ? EX_ZERO3 : 84 + g;       // s_vec rows g, 4 + g, 8 + g of racc_diag; the factor's lanes: three zeros
    if (l < 3) exA[EX_ZERO3 + 4 * l] = 0.0;
    [[maybe_unused]] double *const pgl = (j < 12) ? Lout + g * 12 + j : (j == 12 ? dlout + g : sample_sink(st, b) + l);
    [[maybe_unused]] const long sgl = (j < 12) ? LSTR : (j == 12 ? USTR : 0);
    double zt[3], dg[3], nwrow[3];                               // [A | B] image and diagonal selectors (FlyCtx), -inv(W)_ii of this lane's rows
#pragma unroll
    for (int r = 0; r < 3; ++r) { zt[r] = pb.Zt[64 * r + l]; dg[r] = (j == 4 * r + g) ? 1.0 : 0.0; nwrow[r] = -pb.Wdg[4 * r + g]; }
    const double kappa = pb.kappa;
    const double coef = -1.0 / (2.0 * theta);

    d4 vA, vB;                                                   // terminal condition (see sweep_dual_body)
    {
        const double *__restrict__ tt = tile0 + (long)N * TSTRIDE;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = 4 * r + g;
            const double te = tt[(j < 12) ? TT_Q + i * 12 + j : TT_QV + i];
            vA[r] = (j <= 12) ? te : 0.0;
        }
        const double t3 = tt[(j < 12) ? TT_QV + j : TT_q];
        vA[3] = (g == 0 && j <= 12) ? (j < 12 ? t3 : 2.0 * t3) : 0.0;
        vB = vA;
    }
    double raccA = 0.0;

    auto load = [&](RTile &tr, const int t) {
        const double2 *__restrict__ q = reinterpret_cast<const double2 *>(rp + (long)t * REC_STEP);
        tr.m01 = q[0];
        tr.m2h = q[1];
        tr.x = tile0[(long)t * TSTRIDE + TS_QR + lx];
        tr.xj = xh[(long)t * XSTR + jc];
        tr.la = Lb[(long)t * LSTR + g * 12 + jc] * m12;
    };
    // one backward step; false: a non-finite operand (nothing of this step is stored)
    auto step = [&](const int t, const RTile &cur) -> bool {
        int l = l_, g = g_, j = j_;
        asm volatile("" : "+v"(l), "+v"(g), "+v"(j));
        d4 cz;
#pragma unroll
        for (int r = 0; r < 3; ++r) cz[r] = fx_diag(zt[r], dg[r], kappa, cur.xj);
        cz[3] = 0.0;
        double probe = (cz[0] + cz[1]) + cz[2];
        probe += (vA[0] + vA[1]) + (vA[2] + vA[3]);
        if (GAINB) probe += (vB[0] + vB[1]) + (vB[2] + vB[3]);
        if (__ballot(!(probe - probe == 0.0))) return false;
        const double m0 = cur.m01.x, m1 = cur.m01.y, m2 = cur.m2h.x, gh = cur.m2h.y;
        // column 12 of the three -M^-1 words is the recorded factor of H (layout.h: REC_FACT_*), not matrix data: handed to every lane
        // through the exchange area.  What those lanes feed takes no bit from a finite value there: rows 12..15 of Y, which nothing reads,
        // and racc through nth12 = 0 -- against zeros (sro), so that the sum stays finite whatever s_vec is
        if (GAINB && FACT) { exB[fwo] = m0; exB[fwo + 1] = m1; exB[fwo + 2] = m2; }
        exA[svo] = vA[3];
        if (GAINB) exB[svo] = vB[3];
        // theta s_vec' M^-1 s_vec (:387) of the evaluation (a gain sweep's own value is not used by step!)
        raccA = racc_diag(raccA, nth12, exA[84 + j], m0, m1, m2, exA[sro], exA[sro + 4], exA[sro + 8]);
        d4 mw;
        mw[0] = m0 * nwrow[0]; mw[1] = m1 * nwrow[1]; mw[2] = m2 * nwrow[2]; mw[3] = 0.0;
        const d4 y2 = mm3(mw, cz, (d4){0, 0, 0, 0});
        double tA12, tB12 = 0.0;                                 // row 12 of T (lanes g == 0)
        if (GAINB && STACK) {
            d4 vS;
#pragma unroll
            for (int r = 0; r < 3; ++r) vS[r] = row_ror8_merge<0x2>(vA[r], vB[r]);
            vS[3] = 0.0;
            const d4 tm = mm3(vS, y2, (d4){0, 0, 0, 0});
            tA12 = tm[3];
            tB12 = tm[1];
        } else {
            const d4 tmA = mm3(vA, y2, (d4){0, 0, 0, 0});
            tA12 = tmA[3];
            if (GAINB) { const d4 tmB = mm3(vB, y2, (d4){0, 0, 0, 0}); tB12 = tmB[3]; }
        }
        const double fvA = tA12 + cur.x, fvB = tB12 + cur.x;
        exB[g * 16 + j] = gh;
        exA[fbo] = fvA;
        lbuf[l] = cur.la;
        if (GAINB) exB[fbo] = fvB;
        WAVE_SYNC();
        const double h0 = exB[hoff[0]], h1 = exB[hoff[1]], h2 = exB[hoff[2]], h3 = exB[hoff[3]];
        const double qc = readlane_f64(cur.x, 16);
        if (GAINB) {                                             // optimal gains (:372-382)
            const double gaB = fma(gh, m12, exB[gaoff]);
            const double g0 = exB[goff[0]], g1 = exB[goff[1]], g2 = exB[goff[2]], g3 = exB[goff[3]];
            double l10, l20, l30, l21, l31, l32, i0, i1, i2, i3;
            if (FACT) {                                          // the factor the recorded pass formed from these very H (d1, d2: not needed)
                const double *const fx = exB + EX_FACT;
                l10 = fx[REC_FACT_VAL(0, 0)]; l20 = fx[REC_FACT_VAL(0, 1)]; l30 = fx[REC_FACT_VAL(0, 2)];
                l21 = fx[REC_FACT_VAL(1, 0)]; l31 = fx[REC_FACT_VAL(1, 1)]; l32 = fx[REC_FACT_VAL(1, 2)];
                i0 = fx[REC_FACT_VAL(2, 2)]; i1 = fx[REC_FACT_VAL(3, 0)]; i2 = fx[REC_FACT_VAL(3, 1)]; i3 = fx[REC_FACT_VAL(3, 2)];
            } else {
                const double h00 = exB[12], h01 = exB[13], h02 = exB[14], h03 = exB[15];
                const double h11 = exB[16 + 13], h12 = exB[16 + 14], h13 = exB[16 + 15];
                const double h22 = exB[32 + 14], h23 = exB[32 + 15], h33 = exB[48 + 15];
                const Ldl4 f = ldl4_factor(h00, h01, h02, h03, h11, h12, h13, h22, h23, h33);
                l10 = f.l10; l20 = f.l20; l30 = f.l30; l21 = f.l21; l31 = f.l31; l32 = f.l32; i0 = f.i0; i1 = f.i1; i2 = f.i2; i3 = f.i3;
            }
            const double y0 = -g0;
            const double y1 = -g1 - l10 * y0;
            const double yy2 = -g2 - l20 * y0 - l21 * y1;
            const double y3 = -g3 - l30 * y0 - l31 * y1 - l32 * yy2;
            const double x3 = y3 * i3;
            const double x2 = yy2 * i2 - l32 * x3;
            const double x1 = y1 * i1 - l21 * x2 - l31 * x3;
            const double x0 = y0 * i0 - l10 * x1 - l20 * x2 - l30 * x3;
            const double laB = ((x0 * e00 + x1 * e10) + x2 * e01) + x3 * e11;
            const double uaB = ua_entry(h0, h1, h2, h3, x0, x1, x2, x3, gaB);
            pgl[(long)t * sgl] = (j <= 12) ? laB : 0.0;             // L_t | dl_t | idle lanes: sink
            d4 fxB;
#pragma unroll
            for (int r = 0; r < 3; ++r) fxB[r] = exB[foff[r]];     // column 12 (f_x) exact; the S block is not formed
            fxB[3] = fma(fvB, mA_, (2.0 * qc + vB[3]) * mB_);
            const d4 vn = MFMA(laB, uaB, fxB);
            vB = MFMA(gaB, laB, vn);
        }
        {                                                        // the given policy (:446-451)
            const double gaA = fma(gh, m12, exA[gaoff]);
            const double uaA = ua_entry(h0, h1, h2, h3, lbuf[j], lbuf[16 + j], lbuf[32 + j], lbuf[48 + j], gaA);
            d4 fxA;
#pragma unroll
            for (int r = 0; r < 3; ++r) fxA[r] = exA[foff[r]];
            fxA[3] = fma(fvA, mA_, (2.0 * qc + vA[3]) * mB_);
            const d4 vn = MFMA(cur.la, uaA, fxA);
            vA = MFMA(gaA, cur.la, vn);
        }
        WAVE_SYNC();          // the exchange areas are rewritten next step
        return true;
    };

    RTile r0, r1, r2;
    load(r0, N - 1);
    load(r1, (N > 1) ? N - 2 : 0);
    bool ok = true;
    for (int t = N - 1; t >= 0; t -= 3) {        // (unrolled by three over rotating register sets: the record of step t - 2 is requested at step t)
        load(r2, (t > 1) ? t - 2 : 0);
        if (!step(t, r0)) { ok = false; break; }
        if (t == 0) break;
        load(r0, (t > 2) ? t - 3 : 0);
        if (!step(t - 1, r1)) { ok = false; break; }
        if (t == 1) break;
        load(r1, (t > 3) ? t - 4 : 0);
        if (!step(t - 2, r2)) { ok = false; break; }
    }
    WAVE_SYNC();
    if (!ok) return false;
    const double totA = sweep_scalars(wave_sum(raccA), coef, readlane_f64(v_rprod, 0), __builtin_amdgcn_readfirstlane(v_rexp), true);
    if (l == 12) {
        st.value_c[b * st.E] = 0.5 * vA[3] + totA;
        st.flag_c[b * st.E] = 0;
        if (GAINB) {
            st.mu_spec[b] = mu;                                  // (no restart: mu, Delta unchanged by the gain sweep)
            st.delta_spec[b] = st.delta[b];
            st.spec_st[b] = 1;
            rc.lgen[2 * b + osel] = gen;                         // the gains written are the record's
        }
    }
    if (l == 0) atomicAdd(rc.count + (GAINB ? 0 : 1), GAINB ? 2 : 1);     // [0] sweeps replayed in pairs, [1] last evaluations replayed
    return true;
}
__device__ __forceinline__ bool replay_dual_body(const SweepArgs &a, const int b, double *const wls) {
    if (a.rec.factor) return a.rec.stack ? replay_body<true, true, true>(a, b, wls) : replay_body<true, false, true>(a, b, wls);
    return a.rec.stack ? replay_body<true, true>(a, b, wls) : replay_body<true>(a, b, wls);
}
__device__ __forceinline__ bool replay_eval_body(const SweepArgs &a, const int b, double *const wls) { return replay_body<false>(a, b, wls); }
