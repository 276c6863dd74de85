// passes/hcut.inc — the horizon cut of tiny batches: segment maps, the chain of boundary hops, gains; Gauss-Newton, full Hessian, tracking.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// The tracking gains with the HORIZON cut in segments (VERDICT r3 item 4; aoc_tuning.track_hcut = number of segments).
// The Riccati recursion over the stages [s, e) of a segment is ONE map of the value function at its end,
//     P_s = H + Phi^T P_e (I + Gam P_e)^-1 Phi,
// which the segment builds while walking backward from P_e = 0:  H by the ordinary recursion, and per stage
//     Gam <- Gam + (Phi B) M^-1 (Phi B)^T,   Phi <- Phi (A - B M^-1 G)      (M = R + B^T H B, G = B^T H A)
// (the composition rule of Sarkka & Garcia-Fernandez' parallel-in-time LQR, specialised to "put one stage in front":
// the 6x6 inverse of the general rule collapses to the 2x2 inverse the recursion takes anyway).  Three launches:
//   k_track_hcut_map    grid (tiles, S): segments 0 .. S-2 build their map; the last one, whose end value Q_T is known,
//                       runs the plain recursion (its gains are final) and leaves P at its first stage
//   k_track_hcut_chain  grid (tiles): the value function handed down from segment to segment through the maps
//   k_track_hcut_gains  grid (tiles, S-1): every segment's own recursion and gains from its end value
// Not bit-identical to the sequential kernels (gains agree to ~1e-13 of their scale, tools/probes/horizon_cut_numpy.py).
// Scratch (HcutScratch below is its one description): S maps per tile, then S boundary value functions per tile, then the
// S / 2 composed maps per tile of k_hcut_pair; a map is HC_MAP planes of TILE values, a boundary HC_BND.
// ---------------------------------------------------------------------------------------------
// the planes of a map: H (sym), Phi (row-major), Gam (sym); eta, beta (Newton backward pass only) ...
constexpr int HC_H = 0, HC_PHI = HC_H + 21, HC_GAM = HC_PHI + 36, HC_ETA = HC_GAM + 21, HC_BETA = HC_ETA + 6, HC_MAP = HC_BETA + 6;
// ... and of a boundary value function: P (sym), p
constexpr int HC_BP = 0, HC_Bp = HC_BP + 21, HC_BND = HC_Bp + 6;
// The cut's scratch as the kernels see it: no kernel forms an address in it by itself.  (A map may also sit in LDS,
// k_hcut_chain6: the plane constants and hc_load / hc_store serve both.)
struct HcutScratch {
    real* base;
    int ntiles, S;
    __device__ __forceinline__ HcutScratch(real* scratch, int ntiles_, int S_) : base(scratch), ntiles(ntiles_), S(S_) {}
    // (the gains kernels are handed the scratch read-only)
    __device__ __forceinline__ HcutScratch(const real* scratch, int ntiles_, int S_) : HcutScratch(const_cast<real*>(scratch), ntiles_, S_) {}
    __device__ __forceinline__ real* map(int tile, int seg) const { return base + ((size_t)tile * S + seg) * HC_MAP * TILE; }
    __device__ __forceinline__ real* bnd(int tile, int seg) const {
        return base + (size_t)ntiles * S * HC_MAP * TILE + ((size_t)tile * S + seg) * HC_BND * TILE;
    }
    // composed map k of a tile (k_hcut_pair), behind the boundaries
    __device__ __forceinline__ real* comp(int tile, int k) const {
        return base + (size_t)ntiles * S * (HC_MAP + HC_BND) * TILE + ((size_t)tile * (S / 2) + k) * HC_MAP * TILE;
    }
};
static size_t hcut_scratch_bytes(int ntiles, int S) { return (size_t)ntiles * (S * (HC_MAP + HC_BND) + (S / 2) * HC_MAP) * TILE * sizeof(real); }
// N planes from `plane` on, of a map or a boundary m, to and from registers
template <int N>
__device__ __forceinline__ void hc_load(const real* __restrict__ m, int plane, int lane, real* v) {
#pragma unroll
    for (int e = 0; e < N; e++) v[e] = m[(size_t)(plane + e) * TILE + lane];
}
template <int N>
__device__ __forceinline__ void hc_store(real* __restrict__ m, int plane, int lane, const real* v) {
#pragma unroll
    for (int e = 0; e < N; e++) m[(size_t)(plane + e) * TILE + lane] = v[e];
}
// the value function (P, p) of a boundary b (without AFFINE — tracking — p = 0 and is not stored)
template <bool AFFINE>
__device__ __forceinline__ void hc_load_value(const real* __restrict__ b, int lane, real P[21], real p[6]) {
    hc_load<21>(b, HC_BP, lane, P);
#pragma unroll
    for (int e = 0; e < 6; e++) p[e] = AFFINE ? b[(size_t)(HC_Bp + e) * TILE + lane] : R(0.0);
}
template <bool AFFINE>
__device__ __forceinline__ void hc_store_value(real* __restrict__ b, int lane, const real P[21], const real p[6]) {
    hc_store<21>(b, HC_BP, lane, P);
    if (AFFINE) hc_store<6>(b, HC_Bp, lane, p);
}
// a map in its two halves (see hcut_stage_h / hcut_stage_phi below; eta, beta: nullptr without the affine terms): the
// identity map H = Gam = 0, Phi = I, eta = beta = 0, and the store of a finished one
__device__ __forceinline__ void hc_init_h(real H[21], real* eta) {
#pragma unroll
    for (int e = 0; e < 21; e++) H[e] = R(0.0);
    if (eta) {
#pragma unroll
        for (int e = 0; e < 6; e++) eta[e] = R(0.0);
    }
}
__device__ __forceinline__ void hc_init_phi(real Phi[36], real Gam[21], real* beta) {
#pragma unroll
    for (int e = 0; e < 21; e++) Gam[e] = R(0.0);
#pragma unroll
    for (int e = 0; e < 36; e++) Phi[e] = (e % 7 == 0) ? R(1.0) : R(0.0);
    if (beta) {
#pragma unroll
        for (int e = 0; e < 6; e++) beta[e] = R(0.0);
    }
}
__device__ __forceinline__ void hc_store_h(real* __restrict__ m, int lane, const real H[21], const real* eta) {
    hc_store<21>(m, HC_H, lane, H);
    if (eta) hc_store<6>(m, HC_ETA, lane, eta);
}
__device__ __forceinline__ void hc_store_phi(real* __restrict__ m, int lane, const real Phi[36], const real Gam[21], const real* beta) {
    hc_store<36>(m, HC_PHI, lane, Phi);
    hc_store<21>(m, HC_GAM, lane, Gam);
    if (beta) hc_store<6>(m, HC_BETA, lane, beta);
}
// FULL: is the iterate of this stage not finite?  (a trajectory that diverged earlier: nothing to protect)
__device__ __forceinline__ bool hc_bad_input(const real xs[6], real u0, real u1) {
    const real chk = (u0 + u1) + ((xs[0] + xs[1]) + (xs[2] + xs[3]) + (xs[4] + xs[5]));
    return !(chk - chk == R(0.0));
}
// segment j: stages [cut(j), cut(j+1)).  The last segment only runs the plain recursion, cheaper per stage than a map, so it
// is made AOC_HC_LAST10 tenths of a regular segment long.  Measured (MPC step of 16 tiles): with one wavefront per segment
// (~880 instructions a stage against ~1140) flat from 1.2 to 1.4, with the stage on three / two wavefronts (longest part
// ~575 against ~500) flat from 1.0 to 1.2; one value for both, the cut points are part of the arithmetic.
#ifndef AOC_HC_LAST10
#define AOC_HC_LAST10 11
#endif
__host__ __device__ inline int hcut_cut(int T, int S, int j) { return j >= S ? T - 1 : (int)(((long)(T - 1) * j * 10) / (10 * (S - 1) + AOC_HC_LAST10)); }
// segments a batch of `ntiles` tiles is cut in: the knob (> 0), or by itself (-1): as many as leave every segment
// wavefront a SIMD of its own — 16 up to 64 tiles, 8 up to 128 (measured at 80-128 tiles: Gauss-Newton iteration -9 %,
// MPC step -10 %; 4 segments at 129-256 tiles lose to the sequential multi-wavefront kernels) —, else none.
// full_hessian: the cut of full-Hessian passes stays with batches of at most 64 tiles (far from the optimum it hands lanes
// to the sequential kernel, and at 65-128 tiles that costs more than the cut saves: random starts 1.07 -> 1.20 ms).
static int hcut_segments(int knob, int ntiles, bool full_hessian = false) {
    return knob >= 0 ? knob : (ntiles <= 64 ? 16 : (ntiles <= 128 && !full_hessian) ? 8 : 0);
}
// the segment kernels on three / two wavefronts per (tile, segment) (k_*_hcut_map3, k_*_hcut_gains2; aoc_tuning.hcut_waves:
// 0 never, 1 where every workgroup gets a CU of its own — tiles x segments <= 256: a wavefront of a map kernel holds more than
// half of a SIMD's registers —, 2 always).  Bit-identical either way.
static bool hcut_multiwave(int knob, int ntiles, int S) { return knob >= 2 || (knob == 1 && ntiles * S <= 256); }

// symmetric 6x6 stored as upper triangle
__device__ __forceinline__ real hc_sym(const real* P, int i, int j) { return i <= j ? P[sidx(i, j)] : P[sidx(j, i)]; }

// one stage put in front of a segment map (H, Phi, Gam); see above.  AFFINE (the Newton iteration's backward pass: stage
// cost gradients hq = q/2, hr = r/2) also carries eta (the affine term of the value function from p_e = 0, by the ordinary
// recursion) and the drift  beta <- beta + (Phi B) sigma,  sigma = -M^-1 (B^T eta + r/2):
//     p_s = eta + Phi^T (I + P_e Gam)^-1 (p_e + P_e beta).
// FULL (round 5, full-Hessian iterations): the stage's Q already holds the Hessian terms (Qb = Q + fxx . lambda) and the cross
// term S = fux . lambda (row 0: s02, s03, s05) enters G = B^T H A + S; fl.regularised reports a stage whose M = R + B^T H B
// (H: the segment's own value function from zero) is not positive definite, fl.singular one whose M is singular or
// ill-conditioned — the map is then not trusted for that lane (k_backward2 with `only_tiles`).
// The stage in two halves, so that two wavefronts can share it (k_hcut_map3): everything that hangs on H (hcut_stage_h: M,
// M^-1, the rows of A_cl = A - B M^-1 G, the affine gain, then the ordinary recursion for H and eta) and everything that
// hangs on Phi (hcut_stage_phi: Gam, beta, Phi).  HcutMid is what crosses from the first to the second.
struct HcutMid {
    real i00, i01, i11;          // M^-1
    real r2[6], r4[6], r5[6];    // rows 2, 4, 5 of A_cl (the others are those of A)
    real s0, s1;                 // sigma = -M^-1 (B^T eta + r/2)    (AFFINE)
    real a02, a12, a05, a15, b20, b50;   // the entries of the Jacobians the Phi half needs
};
template <typename F>
__device__ __forceinline__ void hcut_mid_fields(HcutMid& m, F f) {
    f(0, m.i00); f(1, m.i01); f(2, m.i11);
#pragma unroll
    for (int j = 0; j < 6; j++) { f(3 + j, m.r2[j]); f(9 + j, m.r4[j]); f(15 + j, m.r5[j]); }
    f(21, m.s0); f(22, m.s1); f(23, m.a02); f(24, m.a12); f(25, m.a05); f(26, m.a15); f(27, m.b20); f(28, m.b50);
}
constexpr int HC_MID_NF = 29;

template <bool AFFINE, bool FULL = false>
__device__ __forceinline__ void hcut_stage_h(const KConst& k, const Lin& l, real H[21], const real Qb[21], StageFlags& fl,
                                             HcutMid& m, real* eta = nullptr, const real* hq = nullptr,
                                             const real* hr = nullptr, real s02 = R(0.0), real s03 = R(0.0), real s05 = R(0.0)) {
    // rows 2, 4, 5 of W = H A
    real w[3][6];
    constexpr int rows[3] = {2, 4, 5};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int r = rows[a];
        const real h0 = hc_sym(H, r, 0), h1 = hc_sym(H, r, 1), h2 = hc_sym(H, r, 2), h3 = hc_sym(H, r, 3), h4 = hc_sym(H, r, 4),
                   h5 = hc_sym(H, r, 5);
        w[a][0] = h0; w[a][1] = h1;
        w[a][2] = h0 * l.a02 + h1 * l.a12 + h2 * l.a22 + h5 * l.a52;
        w[a][3] = h2 * l.a23 + h3 + h5 * l.a53;
        w[a][4] = h3 * k.dt + h4;
        w[a][5] = h0 * l.a05 + h1 * l.a15 + h2 * l.a25 + h5 * l.a55;
    }
    const real H22 = H[sidx(2, 2)], H24 = H[sidx(2, 4)], H25 = H[sidx(2, 5)], H44 = H[sidx(4, 4)], H45 = H[sidx(4, 5)],
               H55 = H[sidx(5, 5)];
    const real M00 = k.R[0] + ((l.b20 * H22 + l.b50 * H25) * l.b20 + (l.b20 * H25 + l.b50 * H55) * l.b50);
    const real M01 = k.R[1] + (l.b20 * H24 + l.b50 * H45) * k.b41;
    const real M11 = k.R[3] + (k.b41 * H44) * k.b41;
    const real detM = M00 * M11 - M01 * M01;
    const real idet = rcp_fast(detM);
    if (FULL) {
        if (!((M00 + M11 > R(0.0)) && (detM > R(0.0)))) fl.regularised = true;
        // ill-conditioned: |det M| below 1e-9 of the size of its terms (or not a number)
        const real sz = __builtin_fabs(M00 * M11) + M01 * M01;
        if (!(__builtin_fabs(detM) > R(1e-9) * sz)) fl.singular = true;
    }
    m.i00 = M11 * idet; m.i01 = -M01 * idet; m.i11 = M00 * idet;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        real g0 = l.b20 * w[0][j] + l.b50 * w[2][j];
        const real g1 = k.b41 * w[1][j];
        if (FULL) {
            if (j == 2) g0 += s02;
            if (j == 3) g0 += s03;
            if (j == 5) g0 += s05;
        }
        const real mg0 = m.i00 * g0 + m.i01 * g1, mg1 = m.i01 * g0 + m.i11 * g1;
        const real a2 = j == 2 ? l.a22 : j == 3 ? l.a23 : j == 5 ? l.a25 : R(0.0);
        const real a5 = j == 2 ? l.a52 : j == 3 ? l.a53 : j == 5 ? l.a55 : R(0.0);
        const real a4 = j == 4 ? R(1.0) : R(0.0);
        m.r2[j] = a2 - l.b20 * mg0;
        m.r5[j] = a5 - l.b50 * mg0;
        m.r4[j] = a4 - k.b41 * mg1;
    }
    m.s0 = m.s1 = R(0.0);
    if (AFFINE) {
        const real h0 = l.b20 * eta[2] + l.b50 * eta[5] + hr[0], h1 = k.b41 * eta[4] + hr[1];
        m.s0 = -(m.i00 * h0 + m.i01 * h1); m.s1 = -(m.i01 * h0 + m.i11 * h1);
    }
    m.a02 = l.a02; m.a12 = l.a12; m.a05 = l.a05; m.a15 = l.a15; m.b20 = l.b20; m.b50 = l.b50;
    // H <- Q + A^T H A - G^T M^-1 G (and eta): the ordinary stage, no gains kept
    if (AFFINE) {
        const StageFlags f2 = FULL ? lqr_stage(k, l, H, eta, Qb, s02, s03, s05, hq, hr, [](int, real, real) {})
                                   : lqr_stage(k, l, H, eta, Qb, R(0.0), R(0.0), R(0.0), hq, hr, [](int, real, real) {});
        fl.singular |= f2.singular;
    } else {
        real pz[6] = {R(0.0), R(0.0), R(0.0), R(0.0), R(0.0), R(0.0)};
        const real z6[6] = {R(0.0), R(0.0), R(0.0), R(0.0), R(0.0), R(0.0)}, z2[2] = {R(0.0), R(0.0)};
        const StageFlags f2 = lqr_stage(k, l, H, pz, Qb, R(0.0), R(0.0), R(0.0), z6, z2, [](int, real, real) {});
        fl.singular |= f2.singular;
    }
}

template <bool AFFINE>
__device__ __forceinline__ void hcut_stage_phi(const KConst& k, const HcutMid& m, real Phi[36], real Gam[21], real* beta = nullptr) {
    // Gam += (Phi B) M^-1 (Phi B)^T with the OLD Phi
    real c0[6], c1[6], z0[6], z1[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        c0[i] = Phi[i * 6 + 2] * m.b20 + Phi[i * 6 + 5] * m.b50;
        c1[i] = Phi[i * 6 + 4] * k.b41;
        z0[i] = c0[i] * m.i00 + c1[i] * m.i01;
        z1[i] = c0[i] * m.i01 + c1[i] * m.i11;
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Gam[sidx(i, j)] += c0[i] * z0[j] + c1[i] * z1[j];
    if (AFFINE) {
#pragma unroll
        for (int i = 0; i < 6; i++) beta[i] += c0[i] * m.s0 + c1[i] * m.s1;
    }
    // Phi <- Phi A_cl, row by row
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const real f0 = Phi[i * 6 + 0], f1 = Phi[i * 6 + 1], f2 = Phi[i * 6 + 2], f3 = Phi[i * 6 + 3], f4 = Phi[i * 6 + 4],
                   f5 = Phi[i * 6 + 5];
        real n[6];
#pragma unroll
        for (int j = 0; j < 6; j++) n[j] = f2 * m.r2[j] + f4 * m.r4[j] + f5 * m.r5[j];
        n[0] += f0;
        n[1] += f1;
        n[2] += f0 * m.a02 + f1 * m.a12;
        n[3] += f3;
        n[4] += f3 * k.dt;
        n[5] += f0 * m.a05 + f1 * m.a15;
#pragma unroll
        for (int j = 0; j < 6; j++) Phi[i * 6 + j] = n[j];
    }
}

// one stage put in front of a segment map, both halves in one wavefront
template <bool AFFINE, bool FULL = false>
__device__ __forceinline__ void hcut_stage(const KConst& k, const Lin& l, real H[21], real Phi[36], real Gam[21],
                                           const real Qb[21], StageFlags& fl, real* eta = nullptr, real* beta = nullptr,
                                           const real* hq = nullptr, const real* hr = nullptr, real s02 = R(0.0),
                                           real s03 = R(0.0), real s05 = R(0.0)) {
    HcutMid m;
    hcut_stage_h<AFFINE, FULL>(k, l, H, Qb, fl, m, eta, hq, hr, s02, s03, s05);
    hcut_mid_fields(m, [](int, real& v) { bw_opaque(v); });   // the cut between the wavefronts of k_*_hcut_map3: same roundings here
    hcut_stage_phi<AFFINE>(k, m, Phi, Gam, beta);
}

// the plain recursion from (P, p = 0) over the stages t_hi-1 .. t_lo of a tile on ONE wavefront, gains stored: the last segment of
// k_track_hcut_map and every segment of k_track_hcut_gains (hcut_track_recursion below is its LDS-fed counterpart)
template <typename XT>
__device__ __forceinline__ int hcut_track_segment(const KConst& k, const XT* __restrict__ x, const real* __restrict__ u,
                                                  const real* __restrict__ x_opt0, int tile, int lane, int t_lo, int t_hi,
                                                  real P[21], real* __restrict__ Kout) {
    const int T = k.T;
    real p[6], Qb[21], xs[6];
    int flags = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) p[i] = R(0.0);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
    StageIn<XT> cur, nxt;
    real x0r[6];
    stage_x0(x_opt0, tile, lane, t_lo, x0r);
    stage_fetch<false>(x, u, tile, T, t_hi - 1, lane, cur);
    for (int t = t_hi - 1; t >= t_lo; t--) {
        stage_fetch<false>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
        stage_state(cur, x0r, t, xs);
        const SC s = trig(xs[3], xs[5]);
        Lin l = linearise(k, xs, cur.u0, s);
        track_lin_fields(l, [](int, real& v) { bw_opaque(v); });   // the cut of k_track_hcut_map3 / _gains2: same roundings
        flags |= track_gain_stage(k, l, P, p, Qb, Kout, tile, T, t, lane);
        cur = nxt;
    }
    return flags;
}

template <bool DIAG, typename XT>
__global__ __launch_bounds__(TILE) void k_track_hcut_map(KConst k, int S, const XT* __restrict__ x,
                                                         const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                         real* __restrict__ Kout, real* __restrict__ scratch,
                                                         int* __restrict__ status) {
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x, T = k.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);   // stages t_hi-1 .. t_lo
    const HcutScratch hs(scratch, gridDim.x, S);
    real* const maps = hs.map(tile, seg);
    real* const bnd = hs.bnd(tile, seg);
    int flags = 0;
    if (seg == S - 1) {   // the last segment: the plain recursion from Q_T, its gains are final; P at its first stage out
        real P[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) P[sidx(i, j)] = k.QT[i * 6 + j];
        flags = hcut_track_segment(k, x, u, x_opt0, tile, lane, t_lo, t_hi, P, Kout);
        hc_store<21>(bnd, HC_BP, lane, P);
#pragma unroll
        for (int j = 0; j < 12; j++) Kout[tix<12>(tile, T, T - 1, j, lane)] = R(0.0);  // KK[:,:,T-1] stays 0 (:700)
    } else {
        real H[21], Phi[36], Gam[21], Qb[21], xs[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
        hc_init_h(H, nullptr);
        hc_init_phi(Phi, Gam, nullptr);
        StageFlags fl{false, false};
        StageIn<XT> cur, nxt;
        real x0r[6];
        stage_x0(x_opt0, tile, lane, t_lo, x0r);
        stage_fetch<false>(x, u, tile, T, t_hi - 1, lane, cur);
        for (int t = t_hi - 1; t >= t_lo; t--) {
            stage_fetch<false>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const SC s = trig(xs[3], xs[5]);
            Lin l = linearise(k, xs, cur.u0, s);
            track_lin_fields(l, [](int, real& v) { bw_opaque(v); });
            hcut_stage<false>(k, l, H, Phi, Gam, Qb, fl);
            cur = nxt;
        }
        if (fl.singular) flags |= AOC_ST_SINGULAR;
        hc_store_h(maps, lane, H, nullptr);
        hc_store_phi(maps, lane, Phi, Gam, nullptr);
    }
    if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
}

// X Y = F for a dense 6x6 X and NR right-hand sides (Gaussian elimination with partial pivoting, per lane), Y overwrites F.
// Every column of F goes through the same operations whatever NR is: solving one column at a time (k_hcut_chain6) gives
// the bits of solving all six at once (k_track_hcut_chain).
template <int NR>
__device__ __forceinline__ void hc_solve6n(real X[6][6], real F[6][NR]) {
#pragma unroll
    for (int c = 0; c < 6; c++) {
        int piv = c;
        real best = X[c][c] < R(0.0) ? -X[c][c] : X[c][c];
#ifndef AOC_HC_NOPIVOT   // (probe build: the cost of the pivoting, tools/one_kernel.sh ... -DAOC_HC_NOPIVOT)
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            const real v = X[r][c] < R(0.0) ? -X[r][c] : X[r][c];
            if (v > best) { best = v; piv = r; }
        }
#endif
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            const bool sw = piv == r;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const real a = X[c][j], b = X[r][j];
                X[c][j] = sw ? b : a; X[r][j] = sw ? a : b;
            }
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const real e = F[c][j], f = F[r][j];
                F[c][j] = sw ? f : e; F[r][j] = sw ? e : f;
            }
        }
        const real ip = rcp_fast(X[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            const real m = X[r][c] * ip;
#pragma unroll
            for (int j = c + 1; j < 6; j++) X[r][j] -= m * X[c][j];
#pragma unroll
            for (int j = 0; j < NR; j++) F[r][j] -= m * F[c][j];
        }
    }
#pragma unroll
    for (int c = 5; c >= 0; c--) {
        const real ip = rcp_fast(X[c][c]);
#pragma unroll
        for (int j = 0; j < NR; j++) {
            real a = F[c][j];
#pragma unroll
            for (int r = c + 1; r < 6; r++) a -= X[c][r] * F[r][j];
            F[c][j] = a * ip;
        }
    }
}
__device__ __forceinline__ void hc_solve6(real X[6][6], real F[6][6]) { hc_solve6n<6>(X, F); }

// one hop: the value function (P, p) at the END of a segment -> at its first stage, through the segment's map m
// (planes HC_H .. HC_BETA of TILE doubles, in the scratch or in LDS)
template <bool AFFINE>
__device__ __forceinline__ void hcut_hop(const real* __restrict__ m, int lane, real P[21], real p[6]) {
    real X[6][6], F[6][6];
    // X = I + Gam P,  F = Phi
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            real a = i == j ? R(1.0) : R(0.0);
#pragma unroll
            for (int q = 0; q < 6; q++) a += m[(size_t)(HC_GAM + (i <= q ? sidx(i, q) : sidx(q, i))) * TILE + lane] * hc_sym(P, q, j);
            X[i][j] = a;
            F[i][j] = m[(size_t)(HC_PHI + i * 6 + j) * TILE + lane];
        }
    hc_solve6(X, F);                       // F = (I + Gam P)^-1 Phi
    real Z[6][6];                          // Z = P F
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            real a = R(0.0);
#pragma unroll
            for (int q = 0; q < 6; q++) a += hc_sym(P, i, q) * F[q][j];
            Z[i][j] = a;
        }
    if (AFFINE) {   // p <- eta + F^T (p + P beta)   (F^T = Phi^T (I + P Gam)^-1)
        real v[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            real a = p[i];
#pragma unroll
            for (int q = 0; q < 6; q++) a += hc_sym(P, i, q) * m[(size_t)(HC_BETA + q) * TILE + lane];
            v[i] = a;
        }
#pragma unroll
        for (int j = 0; j < 6; j++) {
            real a = m[(size_t)(HC_ETA + j) * TILE + lane];
#pragma unroll
            for (int q = 0; q < 6; q++) a += F[q][j] * v[q];
            p[j] = a;
        }
    }
    // P <- H + Phi^T Z (symmetric part kept as computed for i <= j)
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            real a = m[(size_t)(HC_H + sidx(i, j)) * TILE + lane];
#pragma unroll
            for (int q = 0; q < 6; q++) a += m[(size_t)(HC_PHI + q * 6 + i) * TILE + lane] * Z[q][j];
            P[sidx(i, j)] = a;
        }
}

// The maps of neighbouring segments composed pairwise (aoc_tuning.hcut_pairs; late round 5).  The chain is S - 2 hops in
// series on one wavefront per tile, half of a cut pass once the segment kernels run on several wavefronts.  Two maps compose
// into one of the same form — map 1 the earlier segment [s, m), map 2 the later one [m, e), W = (I + Gam1 H2)^-1:
//     Phi = Phi2 W Phi1,   Gam = Gam2 + Phi2 W Gam1 Phi2^T,   H = H1 + Phi1^T H2 W Phi1,
//     beta = beta2 + Phi2 W (beta1 - Gam1 eta2),   eta = eta1 + Phi1^T W^T (eta2 + H2 beta1)
// (Sarkka & Garcia-Fernandez' combination rule in this file's notation; tools/probes/hcut_compose_maps.py) — so
//   k_hcut_pair   grid (tiles, K) x 2 wavefronts: the K = (S - 2) / 2 pairs (S-3, S-2), (S-5, S-4), ... at once; the two
//                 wavefronts share nothing: one solves for W Phi1 (-> Phi, H, eta), the other for W [Gam1 | beta1 - Gam1 eta2]
//                 (-> Gam, beta), each about a hop's worth of instructions
//   the chain     K hops through the composed maps (every other boundary), then a plain hop if S is odd
//   k_hcut_odd    grid (tiles, K): the boundaries in between, one plain hop each from the boundary behind
// : about K + 2 hop-times in series instead of S - 2 (16 segments: 9 instead of 14).  Another order of the same arithmetic
// (like the cut itself; gains still 1e-14 of their scale from the sequential kernels), decided by the knob and the number
// of segments (by default for cuts in at least 12 segments: hcut_launch_chain), never by the batch in flight.
// Composed maps live behind the boundaries in the scratch (hcut_scratch_bytes).
__host__ __device__ inline int hcut_npairs(int S) { return S >= 4 ? (S - 2) / 2 : 0; }

template <bool AFFINE>
__global__ __launch_bounds__(2 * TILE) void k_hcut_pair(int S, real* __restrict__ scratch) {
    const int tile = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6;
    const int j = S - 2 - 2 * k;                                             // maps j - 1 (earlier: 1) and j (later: 2)
    const HcutScratch hs(scratch, gridDim.x, S);
    const real* __restrict__ m1 = hs.map(tile, j - 1);
    const real* __restrict__ m2 = hs.map(tile, j);
    real* __restrict__ mc = hs.comp(tile, k);
    // every operand is loaded ONCE into registers before the loops that use it (a load inside a loop nest is re-issued per
    // use once a store to the composed map stands between two uses: the first form of this kernel had 640 loads and 500 waits)
    real G1[21], H2[21];
    hc_load<21>(m1, HC_GAM, lane, G1);
    hc_load<21>(m2, HC_H, lane, H2);
    // X = I + Gam1 H2 (both wavefronts: the elimination is the same, only the right-hand sides differ)
    real X[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            real a = i == c ? R(1.0) : R(0.0);
#pragma unroll
            for (int q = 0; q < 6; q++) a += hc_sym(G1, i, q) * hc_sym(H2, q, c);
            X[i][c] = a;
        }
    if (wv == 0) {   // Z = W Phi1;  Phi = Phi2 Z;  H = H1 + Phi1^T (H2 Z);  eta = eta1 + Z^T (eta2 + H2 beta1)
        real Z[6][6];
        hc_load<36>(m1, HC_PHI, lane, &Z[0][0]);
        hc_solve6(X, Z);
        real Y[6][6], v[6];                    // Y = H2 Z,  v = eta2 + H2 beta1
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                real a = R(0.0);
#pragma unroll
                for (int q = 0; q < 6; q++) a += hc_sym(H2, i, q) * Z[q][c];
                Y[i][c] = a;
            }
        if (AFFINE) {
            real b1[6];
            hc_load<6>(m1, HC_BETA, lane, b1);
            hc_load<6>(m2, HC_ETA, lane, v);
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int q = 0; q < 6; q++) v[i] += hc_sym(H2, i, q) * b1[q];
        }
        {
            real F2[36], Fc[36];
            hc_load<36>(m2, HC_PHI, lane, F2);
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    real a = R(0.0);
#pragma unroll
                    for (int q = 0; q < 6; q++) a += F2[i * 6 + q] * Z[q][c];
                    Fc[i * 6 + c] = a;
                }
            hc_store<36>(mc, HC_PHI, lane, Fc);
        }
        real F1[36], Hc[21];
        hc_load<36>(m1, HC_PHI, lane, F1);
        hc_load<21>(m1, HC_H, lane, Hc);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int c = i; c < 6; c++) {
                real a = Hc[sidx(i, c)];
#pragma unroll
                for (int q = 0; q < 6; q++) a += F1[q * 6 + i] * Y[q][c];
                Hc[sidx(i, c)] = a;
            }
        hc_store<21>(mc, HC_H, lane, Hc);
        if (AFFINE) {
            real ec[6];
            hc_load<6>(m1, HC_ETA, lane, ec);
#pragma unroll
            for (int c = 0; c < 6; c++)
#pragma unroll
                for (int q = 0; q < 6; q++) ec[c] += Z[q][c] * v[q];
            hc_store<6>(mc, HC_ETA, lane, ec);
        }
    } else {         // Z = W [Gam1 | beta1 - Gam1 eta2];  Gam = Gam2 + Phi2 Z Phi2^T;  beta = beta2 + Phi2 z
        real Z[6][7];
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int c = 0; c < 6; c++) Z[i][c] = hc_sym(G1, i, c);
            Z[i][6] = R(0.0);
        }
        if (AFFINE) {
            real e2[6];
            hc_load<6>(m2, HC_ETA, lane, e2);
#pragma unroll
            for (int i = 0; i < 6; i++) Z[i][6] = m1[(size_t)(HC_BETA + i) * TILE + lane];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int q = 0; q < 6; q++) Z[i][6] -= hc_sym(G1, i, q) * e2[q];
        }
        hc_solve6n<7>(X, Z);
        real F2[36], Y[6][6], Gc[21];          // Y = Phi2 Z
        hc_load<36>(m2, HC_PHI, lane, F2);
        hc_load<21>(m2, HC_GAM, lane, Gc);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                real a = R(0.0);
#pragma unroll
                for (int q = 0; q < 6; q++) a += F2[i * 6 + q] * Z[q][c];
                Y[i][c] = a;
            }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int c = i; c < 6; c++) {
                real a = Gc[sidx(i, c)];
#pragma unroll
                for (int q = 0; q < 6; q++) a += Y[i][q] * F2[c * 6 + q];
                Gc[sidx(i, c)] = a;
            }
        hc_store<21>(mc, HC_GAM, lane, Gc);
        if (AFFINE) {
            real bc[6];
            hc_load<6>(m2, HC_BETA, lane, bc);
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int q = 0; q < 6; q++) bc[i] += F2[i * 6 + q] * Z[q][6];
            hc_store<6>(mc, HC_BETA, lane, bc);
        }
    }
}

// npairs = 0: S - 2 plain hops; else hcut_npairs(S) hops through the composed maps, then the plain ones that are left
template <bool AFFINE>
__global__ __launch_bounds__(TILE) void k_track_hcut_chain(int S, real* __restrict__ scratch, int npairs) {
    const int tile = blockIdx.x, lane = threadIdx.x;
    const HcutScratch hs(scratch, gridDim.x, S);
    real P[21], p[6];
    hc_load_value<AFFINE>(hs.bnd(tile, S - 1), lane, P, p);                 // at the first stage of the last segment
    int seg = S - 2;
    for (int hop = 0;; hop++) {
        hc_store_value<AFFINE>(hs.bnd(tile, seg), lane, P, p);              // the value function at the END of segment seg
        if (seg == 0) break;                                                // nobody needs P at stage 0
        if (hop < npairs) {
            hcut_hop<AFFINE>(hs.comp(tile, hop), lane, P, p);               // over segments seg - 1 and seg
            seg -= 2;
        } else {
            hcut_hop<AFFINE>(hs.map(tile, seg), lane, P, p);
            seg -= 1;
        }
    }
}

// the boundaries the composed hops stepped over: the END of segment j - 1 from the end of segment j, j = S - 2 - 2k
template <bool AFFINE>
__global__ __launch_bounds__(TILE) void k_hcut_odd(int S, real* __restrict__ scratch) {
    const int tile = blockIdx.x, lane = threadIdx.x, j = S - 2 - 2 * (int)blockIdx.y;
    const HcutScratch hs(scratch, gridDim.x, S);
    real P[21], p[6];
    hc_load_value<AFFINE>(hs.bnd(tile, j), lane, P, p);
    hcut_hop<AFFINE>(hs.map(tile, j), lane, P, p);
    hc_store_value<AFFINE>(hs.bnd(tile, j - 1), lane, P, p);
}

// The chain on several wavefronts per tile (round 5; the kernel keeps the name of its first form, k_hcut_chain6).  A hop of
// k_track_hcut_chain is ~1500 instructions of ONE wavefront (dense 6x6: I + Gam P, an LU with pivoting, three products),
// fifteen hops in series: 40 % of a cut backward pass.  The six columns of (I + Gam P)^-1 Phi, of Z = P F and of the new P
// are independent of one another once X = I + Gam P is known: a column wavefront computes its columns of X, all meet (LDS +
// one barrier), each runs the elimination on the whole X but carries only ITS right-hand sides (columns of Phi), forms its
// columns of Z, of the new P and its entries of the new p, and they meet again for the new value function.  Same
// expressions entry by entry as the one-wavefront kernel (hc_solve6n): bit-identical.
template <bool AFFINE, int J0>
__device__ __forceinline__ void hcut_hop_cols(const real* __restrict__ m, int lane, const real P[21], const real p[6],
                                              real (*shX)[6][TILE], real (*shP)[TILE]) {
    // columns J0, J0 + 1 of X = I + Gam P
#pragma unroll
    for (int c = 0; c < 2; c++) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            real a = i == J0 + c ? R(1.0) : R(0.0);
#pragma unroll
            for (int q = 0; q < 6; q++) a += m[(size_t)(HC_GAM + (i <= q ? sidx(i, q) : sidx(q, i))) * TILE + lane] * hc_sym(P, q, J0 + c);
            shX[J0 + c][i][lane] = a;
        }
    }
    __syncthreads();
    real X[6][6], f[6][2];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) X[i][j] = shX[j][i][lane];
        f[i][0] = m[(size_t)(HC_PHI + i * 6 + J0) * TILE + lane];        // Phi[i][J0], Phi[i][J0 + 1]
        f[i][1] = m[(size_t)(HC_PHI + i * 6 + J0 + 1) * TILE + lane];
    }
    hc_solve6n<2>(X, f);                                             // columns J0, J0 + 1 of (I + Gam P)^-1 Phi
    real v[6];
    if (AFFINE) {   // v = p + P beta
#pragma unroll
        for (int i = 0; i < 6; i++) {
            real a = p[i];
#pragma unroll
            for (int q = 0; q < 6; q++) a += hc_sym(P, i, q) * m[(size_t)(HC_BETA + q) * TILE + lane];
            v[i] = a;
        }
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        constexpr int dummy = 0; (void)dummy;
        const int J = J0 + c;
        real z[6];                                                   // column J of Z = P F
#pragma unroll
        for (int i = 0; i < 6; i++) {
            real a = R(0.0);
#pragma unroll
            for (int q = 0; q < 6; q++) a += hc_sym(P, i, q) * f[q][c];
            z[i] = a;
        }
        if (AFFINE) {   // p_J <- eta_J + F[:, J]^T (p + P beta)
            real a = m[(size_t)(HC_ETA + J) * TILE + lane];
#pragma unroll
            for (int q = 0; q < 6; q++) a += f[q][c] * v[q];
            shP[HC_Bp + J][lane] = a;
        }
        // entries (i, J), i <= J, of P <- H + Phi^T Z
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (i > J) continue;
            real a = m[(size_t)(HC_H + sidx(i, J)) * TILE + lane];
#pragma unroll
            for (int q = 0; q < 6; q++) a += m[(size_t)(HC_PHI + q * 6 + i) * TILE + lane] * z[q];
            shP[HC_BP + sidx(i, J)][lane] = a;
        }
    }
}

// Four wavefronts per tile, one per SIMD of the CU: three take two columns each, the fourth is a LOADER.  (Six column
// wavefronts — and seven with the loader — were tried first: two of them then share a SIMD and the hop takes as long as
// the slowest, 72 us for the chain either way, no faster than one wavefront; so does a hop whose operands, the segment's map
// of 90 doubles per lane, come from global memory inside the hop: each of its three phases then begins with a trip to
// memory.)  The loader copies the map of the NEXT hop into LDS while the others work on this one.
// MEASURED (4096 trajectories, 15 hops): 102 us against 73 us for the one-wavefront kernel — 6.8 us per hop where the
// instruction counts promised 2.5: not the default (aoc_tuning.hcut_chain6 = 0); kept as a tested, bit-identical variant and
// as the record of the attempt (EXPERIMENTS.md).
template <bool AFFINE>
__global__ __launch_bounds__(4 * TILE) void k_hcut_chain6(int S, real* __restrict__ scratch) {
    __shared__ real shM[2][HC_MAP][TILE];     // the maps of this hop and of the next one
    __shared__ real shX[6][6][TILE];          // X = I + Gam P: [column][row][lane]
    __shared__ real shP[HC_BND][TILE];        // the new value function: P (upper triangle), p
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wj = threadIdx.x >> 6;   // wavefront wj < 3 owns columns 2 wj, 2 wj + 1; 3 loads
    const HcutScratch hs(scratch, gridDim.x, S);
    constexpr int NV = AFFINE ? HC_MAP : HC_ETA;   // values of a map that are used
    auto stage_map = [&](int seg, int buf) {   // loader: map of segment seg -> shM[buf]
        const real* m = hs.map(tile, seg);
#pragma unroll 6
        for (int e = 0; e < NV; e++) shM[buf][e][lane] = m[(size_t)e * TILE + lane];
    };
    real P[21], p[6];
    if (wj < 3) {
        hc_load_value<AFFINE>(hs.bnd(tile, S - 1), lane, P, p);            // at the first stage of the last segment
    } else if (S >= 3) {
        stage_map(S - 2, 0);
    }
    __syncthreads();
    int buf = 0;
    for (int seg = S - 2; seg >= 0; seg--, buf ^= 1) {
        if (wj == 0) hc_store_value<AFFINE>(hs.bnd(tile, seg), lane, P, p);   // the value function at the END of segment seg
        if (seg == 0) break;                                              // nobody needs P at stage 0
        const real* m = &shM[buf][0][0];
        switch (wj) {   // wave-uniform: the columns are compile-time indices into the register arrays
            case 0: hcut_hop_cols<AFFINE, 0>(m, lane, P, p, shX, shP); break;
            case 1: hcut_hop_cols<AFFINE, 2>(m, lane, P, p, shX, shP); break;
            case 2: hcut_hop_cols<AFFINE, 4>(m, lane, P, p, shX, shP); break;
            default:   // the loader: the next hop's map into the other buffer, then the barrier inside hcut_hop_cols
                if (seg - 1 >= 1) stage_map(seg - 1, buf ^ 1);
                __syncthreads();
                break;
        }
        __syncthreads();
        if (wj < 3) {   // the new value function, laid out in LDS like a boundary
#pragma unroll
            for (int e = 0; e < 21; e++) P[e] = shP[HC_BP + e][lane];
            if (AFFINE) {
#pragma unroll
                for (int e = 0; e < 6; e++) p[e] = shP[HC_Bp + e][lane];
            }
        }
    }
}

template <bool DIAG, typename XT>
__global__ __launch_bounds__(TILE) void k_track_hcut_gains(KConst k, int S, const XT* __restrict__ x,
                                                           const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                           real* __restrict__ Kout, const real* __restrict__ scratch,
                                                           int* __restrict__ status) {
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x, T = k.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);
    const HcutScratch hs(scratch, gridDim.x, S);
    real P[21];
    hc_load<21>(hs.bnd(tile, seg), HC_BP, lane, P);
    const int flags = hcut_track_segment(k, x, u, x_opt0, tile, lane, t_lo, t_hi, P, Kout);
    if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
}

// ---------------------------------------------------------------------------------------------
// The segment kernels on several wavefronts per (tile, segment) (round 5).  A stage of a map is ~1140 instructions of one
// wavefront (linearisation ~300, H half ~500, Phi half ~350), a stage of the plain recursion ~880; with at most 16 tiles
// (16 x 16 segments = 256 workgroups, one per CU) every wavefront of
//   k_track_hcut_map3    grid (tiles, S) x 3 wavefronts: linearisation one stage ahead | hcut_stage_h | hcut_stage_phi a
//                        stage behind, Lin and HcutMid handed on through LDS (double-buffered, one barrier per stage); the
//                        last segment: linearisation | plain recursion, the third wavefront ends at once
//   k_track_hcut_gains2  grid (tiles, S - 1) x 2 wavefronts: linearisation | recursion and gains
// still has a SIMD of its own and the stage lasts as long as its longest part.  Same expressions, same roundings as the
// one-wavefront kernels (the values that cross a cut are opaque to the compiler there): bit-identical, a scheduling choice.
// ---------------------------------------------------------------------------------------------
// the producer role of both: stages t_hi-1 .. t_lo of `tile`, Lin of the stage of step j into sh[j & 1]; n + extra barriers
template <typename XT>
__device__ __forceinline__ void hcut_track_producer(const KConst& k, const TrigK<real>& tk, const XT* __restrict__ x,
                                                    const real* __restrict__ u, const real* __restrict__ x_opt0, int tile,
                                                    int lane, int t_lo, int t_hi, int extra, real (*sh)[6][TILE][2]) {
    const int T = k.T, n = t_hi - t_lo;
    StageIn<XT> cur, nxt;
    real x0r[6], xs[6];
    stage_x0(x_opt0, tile, lane, t_lo, x0r);
    stage_fetch<false>(x, u, tile, T, t_hi - 1, lane, cur);
    for (int j = 0; j < n + extra; j++) {
        if (j < n) {
            const int t = t_hi - 1 - j;
            stage_fetch<false>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const SC s = trig(xs[3], xs[5], tk);
            Lin l = linearise(k, xs, cur.u0, s);
            real(*dst)[TILE][2] = sh[j & 1];
            track_lin_fields(l, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            cur = nxt;
        }
        __syncthreads();
    }
}
// the plain recursion from (P, p = 0) over the same stages, one step behind the producer; gains stored
__device__ __forceinline__ int hcut_track_recursion(const KConst& k, int tile, int lane, int t_lo, int t_hi, real P[21],
                                                    real* __restrict__ Kout, real (*sh)[6][TILE][2]) {
    const int T = k.T, n = t_hi - t_lo;
    real p[6], Qb[21];
    int flags = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) p[i] = R(0.0);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
    for (int j = 0; j < n + 1; j++) {
        if (j >= 1) {
            const int t = t_hi - j;
            Lin l;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            track_lin_fields(l, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
            flags |= track_gain_stage(k, l, P, p, Qb, Kout, tile, T, t, lane);
        }
        __syncthreads();
    }
    return flags;
}

template <bool DIAG, typename XT>
__global__ __launch_bounds__(3 * TILE) void k_track_hcut_map3(KConst kc, int S, const XT* __restrict__ x,
                                                              const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                              real* __restrict__ Kout, real* __restrict__ scratch,
                                                              int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real shL[2][6][TILE][2];
    __shared__ __attribute__((aligned(16))) real shM[2][(HC_MID_NF + 1) / 2][TILE][2];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = kc.T;
    const bool last = seg == S - 1;
    if (last && wv == 2) return;   // (a barrier waits for the wavefronts that are still there)
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1), n = t_hi - t_lo;
    const HcutScratch hs(scratch, gridDim.x, S);
    real* const maps = hs.map(tile, seg);
    real* const bnd = hs.bnd(tile, seg);
    KConst k = kc;
    if (wv == 0) {   // linearisation, one stage ahead of the others
        TrigK<real> tk;
        if (AOC_PIN) { pin_model(k); pin_trig(tk); }
        hcut_track_producer(k, tk, x, u, x_opt0, tile, lane, t_lo, t_hi, last ? 1 : 2, shL);
        return;
    }
    if (AOC_PIN) pin_consts<DIAG>(k);
    if (last) {   // the plain recursion from Q_T: its gains are final; P at its first stage out
        real P[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) P[sidx(i, j)] = k.QT[i * 6 + j];
        const int flags = hcut_track_recursion(k, tile, lane, t_lo, t_hi, P, Kout, shL);
        hc_store<21>(bnd, HC_BP, lane, P);
#pragma unroll
        for (int j = 0; j < 12; j++) Kout[tix<12>(tile, T, T - 1, j, lane)] = R(0.0);  // KK[:,:,T-1] stays 0 (:700)
        if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
        return;
    }
    if (wv == 1) {   // the H half, one step behind the producer
        real H[21], Qb[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
        hc_init_h(H, nullptr);
        StageFlags fl{false, false};
        for (int j = 0; j < n + 2; j++) {
            if (j >= 1 && j <= n) {
                Lin l;
                real(*src)[TILE][2] = shL[(j - 1) & 1];
                track_lin_fields(l, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
                HcutMid m;
                hcut_stage_h<false>(k, l, H, Qb, fl, m);
                real(*dst)[TILE][2] = shM[j & 1];
                hcut_mid_fields(m, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
        }
        hc_store_h(maps, lane, H, nullptr);
        if (status && fl.singular) atomicOr(&status[tile * TILE + lane], (int)AOC_ST_SINGULAR);
    } else {         // the Phi half, two steps behind
        real Phi[36], Gam[21];
        hc_init_phi(Phi, Gam, nullptr);
        for (int j = 0; j < n + 2; j++) {
            if (j >= 2) {
                HcutMid m;
                real(*src)[TILE][2] = shM[(j - 1) & 1];
                hcut_mid_fields(m, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
                hcut_stage_phi<false>(k, m, Phi, Gam);
            }
            __syncthreads();
        }
        hc_store_phi(maps, lane, Phi, Gam, nullptr);
    }
}

template <bool DIAG, typename XT>
__global__ __launch_bounds__(2 * TILE) void k_track_hcut_gains2(KConst kc, int S, const XT* __restrict__ x,
                                                                const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                                real* __restrict__ Kout, const real* __restrict__ scratch,
                                                                int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real shL[2][6][TILE][2];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = kc.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);
    KConst k = kc;
    if (wv == 0) {
        TrigK<real> tk;
        if (AOC_PIN) { pin_model(k); pin_trig(tk); }
        hcut_track_producer(k, tk, x, u, x_opt0, tile, lane, t_lo, t_hi, 1, shL);
        return;
    }
    if (AOC_PIN) pin_consts<DIAG>(k);
    real P[21];
    hc_load<21>(HcutScratch(scratch, gridDim.x, S).bnd(tile, seg), HC_BP, lane, P);
    const int flags = hcut_track_recursion(k, tile, lane, t_lo, t_hi, P, Kout, shL);
    if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
}

// ---------------------------------------------------------------------------------------------
// The horizon cut for FULL-HESSIAN iterations (round 5; VERDICT r4 item 4; optcon.py:443-451, :461).  The quadratisation of
// stage t needs the costate lambda_{t+1} (Q += fxx . lambda, S = fux . lambda), and the costate is a recursion of its own,
//     lambda_t = A_t^T lambda_{t+1} + q_t,     lambda_{T-1} = q_f,
// LINEAR in lambda and independent of the value function: over a segment [s, e)  lambda_s = M lambda_e + c  with
// M <- A_t^T M, c <- A_t^T c + q_t walking backward from (I, 0).  So a full-Hessian backward pass of a tiny batch is
//   k_bw_hcut_lam        grid (tiles, S)    the costate map (M, c) of every segment (the last one: lambda itself from q_f)
//   k_bw_hcut<.., FULL>  grid (tiles, S)    lambda at the segment's end from the maps behind it (a few 6x6 products), then
//                                           the segment's value-function map with the Hessian terms (hcut_stage<true, true>);
//                                           the last segment runs the plain recursion, its gains are final
//   k_hcut_chain6        grid (tiles)       the boundary value functions, as for Gauss-Newton
//   k_bw_hcut<.., FULL, gains>              every segment's recursion and gains from its boundary, lambda recomputed alongside
//   k_backward2<.., only_tiles>             the SEQUENTIAL kernel for the tiles the cut does not trust, flags merged for the others
// Trust: far from the optimum the full Hessian makes M = R + B^T P B indefinite, the reference regularises the gains but not
// the Riccati recursion (Q3) and single trajectories blow up; a map built on the segment's own value function from zero
// would not reproduce those blow-ups trajectory for trajectory.  A TRAJECTORY therefore takes its gains and flags from the
// sequential kernel (bit-identical to an uncut pass) whenever it meets a stage whose M is not positive definite — in a map
// or in the true recursion (where the reference regularises) — or a singular M: the sequential kernel runs on the tiles that
// hold such a lane and commits those lanes only, so that which kernel computes a trajectory is decided by the trajectory
// alone, not by its tile-mates.  Near the optimum (the iterations kk > 8 of perturbed starts, the tail of a converge-mode solve, where these
// tiny batches occur) nothing is flagged and the pass runs on 16 wavefronts per tile instead of two.
// Scratch behind the Gauss-Newton layout (hcut_scratch_bytes): per (tile, segment) the costate map (36 + 6) and lambda at
// the segment's first stage (6); per lane the flags of the cut (merged into `status` at the end); per tile the verdict.
// ---------------------------------------------------------------------------------------------
constexpr int HC_LMAP = 36 + 6, HC_LB = 6;   // a costate map: M (row-major), c
struct HcutFull {
    real* lmap; real* lb; int* lane_flags; int* tile_flag; int trust;
    __device__ __forceinline__ real* lmap_at(int tile, int S, int seg) const { return lmap + ((size_t)tile * S + seg) * HC_LMAP * TILE; }
    __device__ __forceinline__ real* lb_at(int tile, int S, int seg) const { return lb + ((size_t)tile * S + seg) * HC_LB * TILE; }
};
// one walk over that layout: carves it out of `scratch` (if given) and returns its end, the bytes a full-Hessian pass takes
static size_t hcut_full_layout(void* scratch, int ntiles, int S, HcutFull* out) {
    size_t off = hcut_scratch_bytes(ntiles, S);
    auto take = [&](size_t bytes) { char* q = scratch ? (char*)scratch + off : nullptr; off += bytes; return q; };
    HcutFull f;
    f.lmap = (real*)take((size_t)ntiles * S * HC_LMAP * TILE * sizeof(real));
    f.lb = (real*)take((size_t)ntiles * S * HC_LB * TILE * sizeof(real));
    f.lane_flags = (int*)take(align_up((size_t)ntiles * TILE * sizeof(int), 16));
    f.tile_flag = (int*)take(align_up((size_t)ntiles * sizeof(int), 16));
    f.trust = 0;
    if (out) *out = f;
    return off;
}
static size_t hcut_full_scratch_bytes(int ntiles, int S) { return hcut_full_layout(nullptr, ntiles, S, nullptr); }
static HcutFull hcut_full_carve(void* scratch, int ntiles, int S) {
    HcutFull f;
    hcut_full_layout(scratch, ntiles, S, &f);
    return f;
}

template <bool DIAG, bool RPT, typename XT>
__global__ __launch_bounds__(TILE) void k_bw_hcut_lam(KConst k, int S, const real* __restrict__ ref, const XT* __restrict__ x,
                                                      const real* __restrict__ u, const real* __restrict__ x0, HcutFull hf) {
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x, T = k.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);   // stages t_hi-1 .. t_lo
    real xs[6], q[6], r[2], rb[8];
    if (seg == 0) {   // the flags of this pass start from zero (the launches that raise them come later on the stream)
        hf.lane_flags[tile * TILE + lane] = 0;
        if (lane == 0) hf.tile_flag[tile] = 0;
    }
    if (seg == S - 1) {   // lambda itself: lambda_{T-1} = q_f (optcon.py:429-432), then the recursion (optcon.py:461)
        real lam[6];
        load_state(x, x0, tile, T, T - 1, lane, xs);
        term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), lam);
        StageIn<XT> cur, nxt;
        real x0r[6];
        stage_x0(x0, tile, lane, t_lo, x0r);
        stage_fetch<true>(x, u, tile, T, t_hi - 1, lane, cur);
        for (int t = t_hi - 1; t >= t_lo; t--, cur = nxt) {
            stage_fetch<true>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const real u0 = cur.u0, u1 = cur.u1;
            stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
            const SC s = trig(xs[3], xs[5]);
            const Lin l = linearise(k, xs, u0, s);
            real al[6];
            At_vec(k, l, lam, al);
#pragma unroll
            for (int i = 0; i < 6; i++) lam[i] = al[i] + q[i];
        }
        hc_store<6>(hf.lb_at(tile, S, seg), 0, lane, lam);
        return;
    }
    real M[6][6], c[6];      // M[:, j] = column j
#pragma unroll
    for (int i = 0; i < 6; i++) {
        c[i] = R(0.0);
#pragma unroll
        for (int j = 0; j < 6; j++) M[j][i] = i == j ? R(1.0) : R(0.0);
    }
    StageIn<XT> cur, nxt;
    real x0r[6];
    stage_x0(x0, tile, lane, t_lo, x0r);
    stage_fetch<true>(x, u, tile, T, t_hi - 1, lane, cur);
    for (int t = t_hi - 1; t >= t_lo; t--, cur = nxt) {
        stage_fetch<true>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
        stage_state(cur, x0r, t, xs);
        const real u0 = cur.u0, u1 = cur.u1;
        stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
        const SC s = trig(xs[3], xs[5]);
        const Lin l = linearise(k, xs, u0, s);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            real y[6];
            At_vec(k, l, M[j], y);
#pragma unroll
            for (int i = 0; i < 6; i++) M[j][i] = y[i];
        }
        real y[6];
        At_vec(k, l, c, y);
#pragma unroll
        for (int i = 0; i < 6; i++) c[i] = y[i] + q[i];
    }
    real* lm = hf.lmap_at(tile, S, seg);
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) lm[(size_t)(i * 6 + j) * TILE + lane] = M[j][i];      // row-major M[i][j]
        lm[(size_t)(36 + i) * TILE + lane] = c[i];
    }
}

// lambda at the END of segment seg (= at the first stage of segment seg + 1), seg < S - 1: from lambda at the first stage of
// the last segment down through the costate maps of the segments in between
__device__ __forceinline__ void hcut_lambda_end(const HcutFull& hf, int tile, int S, int seg, int lane, real lam[6]) {
    hc_load<6>(hf.lb_at(tile, S, S - 1), 0, lane, lam);
    for (int sgm = S - 2; sgm > seg; sgm--) {
        const real* lm = hf.lmap_at(tile, S, sgm);
        real y[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            real a = lm[(size_t)(36 + i) * TILE + lane];
#pragma unroll
            for (int j = 0; j < 6; j++) a += lm[(size_t)(i * 6 + j) * TILE + lane] * lam[j];
            y[i] = a;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) lam[i] = y[i];
    }
}

// what the segment kernels do with the flags of a lane at the end (FULL: they wait in scratch: a lane the cut does not trust
// gets the sequential kernel's own)
template <bool FULL>
__device__ __forceinline__ void hcut_bw_flags(const HcutFull& hf, int* __restrict__ status, int tile, int lane, int flags,
                                              bool distrust, bool true_recursion) {
    if (FULL) {
        if (distrust) flags |= HC_DISTRUST | (true_recursion ? HC_WHY_TRUE : HC_WHY_MAP);
        if (flags) atomicOr(&hf.lane_flags[tile * TILE + lane], flags);
        if (__ballot(distrust) != 0ull && lane == 0) atomicOr(&hf.tile_flag[tile], 1);
    } else if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
}
// ... and the verdict of a true recursion (last segment, gains pass).  trust 0: a lane whose true recursion regularises or
// meets a singular M; trust 1: the singular ones only (and whatever is not a number: its PD test fails at every stage and
// the value function is checked here)
template <bool FULL>
__device__ __forceinline__ bool hcut_bw_distrust(const HcutFull& hf, int flags, const real P[21], bool bad_in) {
    bool distrust = hf.trust ? (flags & AOC_ST_SINGULAR) != 0 : flags != 0;
    if (FULL && hf.trust) {
        bool finite = true;
#pragma unroll
        for (int e = 0; e < 21; e++) finite = finite && (P[e] - P[e] == R(0.0));
        distrust = (distrust || !finite) && !bad_in;
    }
    return distrust;
}

// The Gauss-Newton backward pass of the Newton iteration with the horizon cut the same way (aoc_tuning.bw_hcut segments):
// affine terms included (hcut_stage<true>), K~ stored as k_backward stores it.
// y = 0: map of a segment (the last one: the plain recursion, gains final); y = 1 (second launch): gains from the boundary.
template <bool DIAG, bool RPT, typename XT, bool GAINS, bool FULL = false>
__global__ __launch_bounds__(TILE) void k_bw_hcut(KConst k, int S, const real* __restrict__ ref, const XT* __restrict__ x,
                                                  const real* __restrict__ u, const real* __restrict__ x0,
                                                  real* __restrict__ Kt, real* __restrict__ scratch, int* __restrict__ status,
                                                  HcutFull hf = HcutFull{nullptr, nullptr, nullptr, nullptr, 0}) {
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x, T = k.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);   // stages t_hi-1 .. t_lo
    const HcutScratch hs(scratch, gridDim.x, S);
    real* const maps = hs.map(tile, seg);
    real* const bnd = hs.bnd(tile, seg);
    real P[21], p[6], lam[6], Qb[21], xs[6];
    int flags = 0;
    bool distrust = false;     // FULL: a stage whose M is not positive definite or singular (see above)
    bool bad_in = false;       // FULL: the iterate itself is not finite (a trajectory that diverged earlier: nothing to protect)
    const bool last = seg == S - 1;
    if (GAINS || !last) {
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
        if (FULL) hcut_lambda_end(hf, tile, S, seg, lane, lam);     // lambda_{t_hi}
    }
    if (GAINS || last) {
        if (GAINS) hc_load_value<true>(bnd, lane, P, p);   // this segment's end value, from the chain
        else bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);
        StageIn<XT> cur, nxt;
        real x0r[6];
        stage_x0(x0, tile, lane, t_lo, x0r);
        stage_fetch<true>(x, u, tile, T, t_hi - 1, lane, cur);
        for (int t = t_hi - 1; t >= t_lo; t--, cur = nxt) {
            stage_fetch<true>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const real u0 = cur.u0, u1 = cur.u1;
            if (FULL) bad_in = bad_in || hc_bad_input(xs, u0, u1);
            BwIn in;
            bw_produce<DIAG, RPT, FULL, FULL>(k, ref, tile, lane, t, xs, u0, u1, lam, in);
            bw_fields<FULL>(in, [](int, real& v) { bw_opaque(v); });   // the cut of k_bw_hcut_map3 / _gains2: same roundings
            bw_derive<FULL>(in);
            const StageFlags fl = bw_consume<FULL>(k, in, P, p, Qb, [&](int c, real a, real b) {
                kt_store<true>(Kt, tile, T, t, c, lane, a, b);
            });
            if (fl.singular) flags |= AOC_ST_SINGULAR;
            if (fl.regularised) flags |= AOC_ST_REGULARISED;
        }
        distrust = hcut_bw_distrust<FULL>(hf, flags, P, bad_in);
        if (!GAINS) hc_store_value<true>(bnd, lane, P, p);   // (P, p) at the first stage of the last segment
    } else {
        real H[21], Phi[36], Gam[21], eta[6], beta[6];
        hc_init_h(H, eta);
        hc_init_phi(Phi, Gam, beta);
        StageFlags fl{false, false};
        StageIn<XT> cur, nxt;
        real x0r[6];
        stage_x0(x0, tile, lane, t_lo, x0r);
        stage_fetch<true>(x, u, tile, T, t_hi - 1, lane, cur);
        for (int t = t_hi - 1; t >= t_lo; t--, cur = nxt) {
            stage_fetch<true>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const real u0 = cur.u0, u1 = cur.u1;
            BwIn in;
            bw_produce<DIAG, RPT, FULL, FULL>(k, ref, tile, lane, t, xs, u0, u1, lam, in);
            bw_fields<FULL>(in, [](int, real& v) { bw_opaque(v); });
            if (FULL) {
                bad_in = bad_in || hc_bad_input(xs, u0, u1);
                bw_derive<true>(in);
                real Qs[21];
                bw_stage_q<true>(in, Qb, Qs);
                hcut_stage<true, true>(k, in.l, H, Phi, Gam, Qs, fl, eta, beta, in.hq, in.hr, in.s02, in.s03, in.s05);
            } else {
                hcut_stage<true>(k, in.l, H, Phi, Gam, Qb, fl, eta, beta, in.hq, in.hr);
            }
        }
        if (fl.singular) flags |= AOC_ST_SINGULAR;
        // (the maps raise no REGULARISED flag: the gains pass reports the true recursion)
        distrust = hf.trust ? (fl.singular && !bad_in) : (fl.singular || fl.regularised);
        hc_store_h(maps, lane, H, eta);
        hc_store_phi(maps, lane, Phi, Gam, beta);
    }
    hcut_bw_flags<FULL>(hf, status, tile, lane, flags, distrust, GAINS || last);
}

// The same on several wavefronts per (tile, segment), see k_track_hcut_map3: k_bw_hcut_map3 (producer: everything bw_produce
// does for a stage, the costate included | H half | Phi half; the last segment: producer | recursion and gains) and
// k_bw_hcut_gains2 (producer | recursion and gains).  Bit-identical to k_bw_hcut.
template <bool DIAG, bool RPT, bool FULL, typename XT, int NF2>
__device__ __forceinline__ bool hcut_bw_producer(const KConst& k, const TrigK<real>& tk, const real* __restrict__ ref,
                                                 const XT* __restrict__ x, const real* __restrict__ u,
                                                 const real* __restrict__ x0, int tile, int lane, int t_lo, int t_hi, int extra,
                                                 real lam[6], real (*sh)[NF2][TILE][2]) {
    const int T = k.T, n = t_hi - t_lo;
    StageIn<XT> cur, nxt;
    real x0r[6], xs[6];
    bool bad_in = false;
    stage_x0(x0, tile, lane, t_lo, x0r);
    stage_fetch<true>(x, u, tile, T, t_hi - 1, lane, cur);
    for (int j = 0; j < n + extra; j++) {
        if (j < n) {
            const int t = t_hi - 1 - j;
            stage_fetch<true>(x, u, tile, T, t > t_lo ? t - 1 : t, lane, nxt);
            stage_state(cur, x0r, t, xs);
            const real u0 = cur.u0, u1 = cur.u1;
            if (FULL) bad_in = bad_in || hc_bad_input(xs, u0, u1);
            BwIn in;
            bw_produce<DIAG, RPT, FULL, FULL>(k, ref, tile, lane, t, xs, u0, u1, lam, in, tk);
            real(*dst)[TILE][2] = sh[j & 1];
            bw_fields<FULL>(in, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            cur = nxt;
        }
        __syncthreads();
    }
    return bad_in;
}
template <bool FULL, int NF2>
__device__ __forceinline__ int hcut_bw_recursion(const KConst& k, int tile, int lane, int t_lo, int t_hi, real P[21], real p[6],
                                                 const real Qb[21], real* __restrict__ Kt, real (*sh)[NF2][TILE][2]) {
    const int T = k.T, n = t_hi - t_lo;
    int flags = 0;
    for (int j = 0; j < n + 1; j++) {
        if (j >= 1) {
            const int t = t_hi - j;
            BwIn in;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            bw_fields<FULL>(in, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
            bw_derive<FULL>(in);
            const StageFlags fl = bw_consume<FULL>(k, in, P, p, Qb, [&](int c, real a, real b) {
                kt_store<true>(Kt, tile, T, t, c, lane, a, b);
            });
            if (fl.singular) flags |= AOC_ST_SINGULAR;
            if (fl.regularised) flags |= AOC_ST_REGULARISED;
        }
        __syncthreads();
    }
    return flags;
}
template <bool DIAG, bool RPT, typename XT, bool FULL>
__global__ __launch_bounds__(3 * TILE) void k_bw_hcut_map3(KConst kc, int S, const real* __restrict__ ref, const XT* __restrict__ x,
                                                           const real* __restrict__ u, const real* __restrict__ x0,
                                                           real* __restrict__ Kt, real* __restrict__ scratch, int* __restrict__ status,
                                                           HcutFull hf) {
    constexpr int NF2 = ((FULL ? BW_NF_FULL : BW_NF_GN) + 1) / 2;
    __shared__ __attribute__((aligned(16))) real shB[2][NF2][TILE][2];
    __shared__ __attribute__((aligned(16))) real shM[2][(HC_MID_NF + 1) / 2][TILE][2];
    __shared__ int shBad[TILE];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = kc.T;
    const bool last = seg == S - 1;
    if (last && wv == 2) return;   // (a barrier waits for the wavefronts that are still there)
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1), n = t_hi - t_lo;
    const HcutScratch hs(scratch, gridDim.x, S);
    real* const maps = hs.map(tile, seg);
    real* const bnd = hs.bnd(tile, seg);
    KConst k = kc;
    real P[21], p[6], lam[6], Qb[21];
    if (wv == 0) {   // everything that depends on the iterate and on the costate only, one stage ahead of the others
        TrigK<real> tk;
        if (AOC_PIN) { pin_consts<DIAG>(k); pin_trig(tk); }
        if (last) bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);
        else if (FULL) hcut_lambda_end(hf, tile, S, seg, lane, lam);     // lambda_{t_hi}
        const bool bad_in = hcut_bw_producer<DIAG, RPT, FULL>(k, tk, ref, x, u, x0, tile, lane, t_lo, t_hi, last ? 1 : 2, lam, shB);
        if (FULL) { shBad[lane] = bad_in; __syncthreads(); }
        return;
    }
    if (AOC_PIN) pin_consts<DIAG>(k);
    if (last) {   // the plain recursion from the terminal condition: its gains are final; (P, p) at its first stage out
        bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);
        const int flags = hcut_bw_recursion<FULL>(k, tile, lane, t_lo, t_hi, P, p, Qb, Kt, shB);
        bool bad_in = false;
        if (FULL) { __syncthreads(); bad_in = shBad[lane] != 0; }
        hc_store_value<true>(bnd, lane, P, p);
        hcut_bw_flags<FULL>(hf, status, tile, lane, flags, hcut_bw_distrust<FULL>(hf, flags, P, bad_in), true);
        return;
    }
    if (wv == 1) {   // the H half (and eta), one step behind the producer
        real H[21], eta[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
        hc_init_h(H, eta);
        StageFlags fl{false, false};
        for (int j = 0; j < n + 2; j++) {
            if (j >= 1 && j <= n) {
                BwIn in;
                real(*src)[TILE][2] = shB[(j - 1) & 1];
                bw_fields<FULL>(in, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
                HcutMid m;
                if (FULL) {
                    bw_derive<true>(in);
                    real Qs[21];
                    bw_stage_q<true>(in, Qb, Qs);
                    hcut_stage_h<true, true>(k, in.l, H, Qs, fl, m, eta, in.hq, in.hr, in.s02, in.s03, in.s05);
                } else {
                    hcut_stage_h<true>(k, in.l, H, Qb, fl, m, eta, in.hq, in.hr);
                }
                real(*dst)[TILE][2] = shM[j & 1];
                hcut_mid_fields(m, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
        }
        bool bad_in = false;
        if (FULL) { __syncthreads(); bad_in = shBad[lane] != 0; }
        hc_store_h(maps, lane, H, eta);
        // (the maps raise no REGULARISED flag: the gains pass reports the true recursion)
        const bool distrust = hf.trust ? (fl.singular && !bad_in) : (fl.singular || fl.regularised);
        hcut_bw_flags<FULL>(hf, status, tile, lane, fl.singular ? (int)AOC_ST_SINGULAR : 0, FULL && distrust, false);
    } else {         // the Phi half (and beta), two steps behind
        real Phi[36], Gam[21], beta[6];
        hc_init_phi(Phi, Gam, beta);
        for (int j = 0; j < n + 2; j++) {
            if (j >= 2) {
                HcutMid m;
                real(*src)[TILE][2] = shM[(j - 1) & 1];
                hcut_mid_fields(m, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
                hcut_stage_phi<true>(k, m, Phi, Gam, beta);
            }
            __syncthreads();
        }
        if (FULL) __syncthreads();
        hc_store_phi(maps, lane, Phi, Gam, beta);
    }
}

template <bool DIAG, bool RPT, typename XT, bool FULL>
__global__ __launch_bounds__(2 * TILE) void k_bw_hcut_gains2(KConst kc, int S, const real* __restrict__ ref, const XT* __restrict__ x,
                                                             const real* __restrict__ u, const real* __restrict__ x0,
                                                             real* __restrict__ Kt, real* __restrict__ scratch, int* __restrict__ status,
                                                             HcutFull hf) {
    constexpr int NF2 = ((FULL ? BW_NF_FULL : BW_NF_GN) + 1) / 2;
    __shared__ __attribute__((aligned(16))) real shB[2][NF2][TILE][2];
    __shared__ int shBad[TILE];
    const int tile = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = kc.T;
    const int t_lo = hcut_cut(T, S, seg), t_hi = hcut_cut(T, S, seg + 1);
    KConst k = kc;
    real lam[6];
    if (wv == 0) {
        TrigK<real> tk;
        if (AOC_PIN) { pin_consts<DIAG>(k); pin_trig(tk); }
        if (FULL) hcut_lambda_end(hf, tile, S, seg, lane, lam);     // lambda_{t_hi}
        const bool bad_in = hcut_bw_producer<DIAG, RPT, FULL>(k, tk, ref, x, u, x0, tile, lane, t_lo, t_hi, 1, lam, shB);
        if (FULL) { shBad[lane] = bad_in; __syncthreads(); }
        return;
    }
    if (AOC_PIN) pin_consts<DIAG>(k);
    real P[21], p[6], Qb[21];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Qb[sidx(i, j)] = k.Q[i * 6 + j];
    hc_load_value<true>(HcutScratch(scratch, gridDim.x, S).bnd(tile, seg), lane, P, p);
    const int flags = hcut_bw_recursion<FULL>(k, tile, lane, t_lo, t_hi, P, p, Qb, Kt, shB);
    bool bad_in = false;
    if (FULL) { __syncthreads(); bad_in = shBad[lane] != 0; }
    hcut_bw_flags<FULL>(hf, status, tile, lane, flags, hcut_bw_distrust<FULL>(hf, flags, P, bad_in), true);
}

template <typename XT, typename XO>
__global__ __launch_bounds__(TILE) void k_track_rollout(KConst k, const XT* __restrict__ x,
                                                        const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                        const real* __restrict__ Kin, const real* __restrict__ x0,
                                                        XO* __restrict__ x_reg, real* __restrict__ u_reg,
                                                        int* __restrict__ status) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real xs[6], xn[6], xo[6];
    int flags = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
        x_reg[tix<6>(tile, T, 0, c, lane)] = (XO)xs[c];
    }
    for (int t = 0; t < T - 1; t++) {
        real d[6], u0, u1;
        load_state(x, x_opt0, tile, T, t, lane, xo);
        {
#pragma clang fp contract(off)
            // uu_reg = uu_opt + KK @ (xx_reg - xx_opt)   (lqr_tracking.py:280)
#pragma unroll
            for (int c = 0; c < 6; c++) d[c] = xs[c] - xo[c];
            real a0 = R(0.0), a1 = R(0.0);
#pragma unroll
            for (int c = 0; c < 6; c++) {
                a0 += Kin[tix<12>(tile, T, t, c, lane)] * d[c];
                a1 += Kin[tix<12>(tile, T, t, 6 + c, lane)] * d[c];
            }
            u0 = u[tix<2>(tile, T, t, 0, lane)] + a0;
            u1 = u[tix<2>(tile, T, t, 1, lane)] + a1;
        }
        if (!(xs[2] > R(0.0))) flags |= AOC_ST_VNONPOS;
        const SC s = trig(xs[3], xs[5]);
        step_state(k, xs, u0, u1, s, xn);
        u_reg[tix<2>(tile, T, t, 0, lane)] = u0;
        u_reg[tix<2>(tile, T, t, 1, lane)] = u1;
#pragma unroll
        for (int c = 0; c < 6; c++) { x_reg[tix<6>(tile, T, t + 1, c, lane)] = (XO)xn[c]; xs[c] = xn[c]; }
    }
    u_reg[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);
    u_reg[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
    if (status && flags) status[tile * TILE + lane] |= flags;
}

