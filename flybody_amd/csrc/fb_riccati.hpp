// fb_batch_lqr_backward: the batched LQR / iLQR backward pass (include/flybody_engine.h).  Dense FP64 linear algebra on
// matrices that do not fit LDS (ndx = 275 for the walking fly), so the horizon loop runs on the host (fb_engine.hip: run_lqr_backward) and
// every interval enqueues a few launches of the four kernels below on the caller's stream:
//
//   k_riccati_gemm   C[m] = op(X[m]) op(Y[m]) (+ D[m]), one wave per 32 x 32 output tile of one nominal, on the FP64 matrix core
//   k_riccati_gain   per nominal: Cholesky of Quu + mu I in LDS, K and k by two triangular solves with one right-hand side per lane,
//                    the vector terms (Qx, Qu, p_t), dV and status
//   k_riccati_sym    P_t = (S + S')/2
//   k_riccati_init   P_T = Qf, p_T = q_T, status = 0, dV = 0
//
// A nominal whose status is non-zero (a pivot of Quu + mu I that is <= 0 or not finite) is skipped by every later launch: its outputs for
// the failing interval and all earlier ones stay zero (the host zeroes the outputs up front, and the gain kernel zeroes what an earlier
// iteration of the stationary mode wrote).
//
// THE TILE PRIMITIVE, ric_tile2x2: four v_mfma_f64_16x16x4_f64 on a 2 x 2 arrangement of 16 x 16 accumulators.  Lane l supplies
// A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] (one double each, the map of the f32 16x16x4 form) and receives, in register r of
// an accumulator, C[row (l >> 4) + 4 r][col l & 15] -- the f64 C/D map, which is NOT the f32 one ((l >> 4)*4 + r).  Under FB_EMULATE
// (x86: no builtin) and under FB_RICCATI_NO_MFMA (a switch of tools/lqr_bench.py's comparison build only) the same interface is plain C++:
// the operands go through LDS and every lane sums its 16 results with fma in ascending k.  Edges (ndx, nu are no multiples of 16 or 4): the
// operand loads are predicated and supply zero outside the matrix; nothing outside a matrix is read or written.
#pragma once

#define FB_RIC_NUMAX 64                    // nu: the solve keeps one right-hand side of FB_RIC_NUMAX doubles in a lane's registers
#define FB_RIC_NDXMAX 1024                 // ndx: the gain kernel keeps Qx in FB_RIC_NDXMAX / FB_RIC_THREADS registers per lane
#define FB_RIC_THREADS 256                 // workgroup of k_riccati_gain / _sym / _init
#define FB_RIC_LD (FB_RIC_NUMAX + 1)       // row stride of the factor in LDS (odd: a column walks all banks)
#define FB_RIC_TILE 32                     // output tile of one k_riccati_gemm wave
#define FB_RIC_KSTEPS 4                    // k-steps of 4 whose operand loads k_riccati_gemm issues together

#if defined(FB_EMULATE) || defined(FB_RICCATI_NO_MFMA)
__device__ __forceinline__ void ric_tile2x2(double a0, double a1, double b0, double b1, double (&c)[2][2][4]) {
  __shared__ double sa[2][64], sb[2][64];
  const int lane = threadIdx.x;
  sa[0][lane] = a0; sa[1][lane] = a1; sb[0][lane] = b0; sb[1][lane] = b1;
  __syncthreads();
  const int col = lane & 15, row0 = lane >> 4;
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int r = 0; r < 4; r++) {
    double s = c[i][j][r];
    for (int k = 0; k < 4; k++) s = fma(sa[i][row0 + 4*r + 16*k], sb[j][col + 16*k], s);
    c[i][j][r] = s;
  }
  __syncthreads();
}
#else
typedef double ric_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void ric_mfma(double a, double b, double (&c)[4]) {
  ric_d4 v = {c[0], c[1], c[2], c[3]};
  v = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, v, 0, 0, 0);
  c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
}
__device__ __forceinline__ void ric_tile2x2(double a0, double a1, double b0, double b1, double (&c)[2][2][4]) {
  ric_mfma(a0, b0, c[0][0]); ric_mfma(a0, b1, c[0][1]); ric_mfma(a1, b0, c[1][0]); ric_mfma(a1, b1, c[1][1]);
}
#endif

// C[m] = op(X[m]) op(Y[m]) (+ D[m]): op(X) is M x K with element (i, k) at X[i*xi + k*xk], op(Y) is K x N with (k, j) at Y[k*yk + j*yj] --
// a transpose is a swap of the two strides --, D and C row-major with ldd / ldc.  s*: the nominal's stride (0: one matrix for all).  D may
// be C (every element is read and written by the same lane).  Grid: n_nom * tm * tn workgroups of one wave.
struct RicGemm {
  const double *X, *Y, *D; double* C;
  long long sX, sY, sD, sC, xi, xk, yk, yj;
  int M, N, K, ldd, ldc, tm, tn;
  const int* status;                       // [n_nom], non-zero: skip the nominal; NULL: none is skipped
};

__global__ void __launch_bounds__(64) k_riccati_gemm(RicGemm g) {
  const int lane = threadIdx.x;
  int bid = blockIdx.x;
  const int tj = bid % g.tn; bid /= g.tn;
  const int ti = bid % g.tm; const int m = bid/g.tm;
  if (g.status && g.status[m] != 0) return;
  const double* X = g.X + m*g.sX; const double* Y = g.Y + m*g.sY;
  const int i0 = ti*FB_RIC_TILE, j0 = tj*FB_RIC_TILE, r = lane & 15, kq = lane >> 4;
  const bool vi0 = i0 + r < g.M, vi1 = i0 + 16 + r < g.M, vj0 = j0 + r < g.N, vj1 = j0 + 16 + r < g.N;
  const double* x0 = X + (long long)(i0 + r)*g.xi; const double* x1 = x0 + 16*g.xi;
  const double* y0 = Y + (long long)(j0 + r)*g.yj; const double* y1 = y0 + 16*g.yj;
  double c[2][2][4] = {};
  // four k-steps at a time: their sixteen loads are in flight together (one step per round trip left the wave waiting on memory);
  // the steps behind K carry zeros on both sides
  for (int k0 = 0; k0 < g.K; k0 += 4*FB_RIC_KSTEPS) {
    double a0[FB_RIC_KSTEPS], a1[FB_RIC_KSTEPS], b0[FB_RIC_KSTEPS], b1[FB_RIC_KSTEPS];
#pragma unroll
    for (int u = 0; u < FB_RIC_KSTEPS; u++) {
      const int k = k0 + 4*u + kq; const bool vk = k < g.K;
      a0[u] = vk && vi0 ? x0[k*g.xk] : 0.0; a1[u] = vk && vi1 ? x1[k*g.xk] : 0.0;
      b0[u] = vk && vj0 ? y0[k*g.yk] : 0.0; b1[u] = vk && vj1 ? y1[k*g.yk] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < FB_RIC_KSTEPS; u++) ric_tile2x2(a0[u], a1[u], b0[u], b1[u], c);
  }
  const double* D = g.D ? g.D + m*g.sD : nullptr; double* C = g.C + m*g.sC;
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int q = 0; q < 4; q++) {
    const int row = i0 + 16*i + kq + 4*q, col = j0 + 16*j + r;             // the f64 C/D map
    if (row < g.M && col < g.N) C[(long long)row*g.ldc + col] = D ? D[(long long)row*g.ldd + col] + c[i][j][q] : c[i][j][q];
  }
}

// One interval of one nominal behind the products.  All pointers are the interval's own (the host adds t); s*: the nominal's stride.
struct RicGain {
  const double *A, *B; long long sA, sB;                 // A_t [ndx][ndx], B_t [ndx][nu]
  const double *Qux, *Quu; long long sQux, sQuu;         // B'W [nu][ndx], R + B'Y [nu][nu] (without mu)
  const double *q, *r; long long sq, sr;                 // q_t [ndx], r_t [nu]; NULL: zero
  const double* mu;                                      // [n_nom]; NULL: zero
  const double* p_next; long long sp_next;               // p_{t+1} [ndx]
  double* p_out; long long sp_out;                       // p_t [ndx]
  double *Kt, *k; long long sKt, sk;                     // K_t transposed [ndx][nu], k_t [nu] (k NULL: not asked for)
  double* dV; int* status;                               // [n_nom][2] (NULL: not asked for), [n_nom]
  int ndx, nu, t;
};

__global__ void __launch_bounds__(FB_RIC_THREADS) k_riccati_gain(RicGain g) {
  __shared__ double L[FB_RIC_NUMAX*FB_RIC_LD];           // Quu + mu I, then its lower Cholesky factor below the diagonal (zero beyond nu)
  __shared__ double dg[FB_RIC_NUMAX], qu[FB_RIC_NUMAX], kv[FB_RIC_NUMAX], gv[FB_RIC_NUMAX], tq[FB_RIC_NUMAX];
  const int tid = threadIdx.x, m = blockIdx.x, ndx = g.ndx, nu = g.nu;
  if (g.status[m] != 0) return;
  const double* A = g.A + m*g.sA; const double* B = g.B + m*g.sB;
  const double* Qux = g.Qux + m*g.sQux; const double* Quu = g.Quu + m*g.sQuu;
  const double* pn = g.p_next + m*g.sp_next;
  double* Kt = g.Kt + m*g.sKt;
  const double mu = g.mu ? g.mu[m] : 0.0;
  for (int e = tid; e < FB_RIC_NUMAX*FB_RIC_LD; e += FB_RIC_THREADS) {
    const int i = e/FB_RIC_LD, j = e % FB_RIC_LD;
    L[e] = i < nu && j < nu ? Quu[i*nu + j] + (i == j ? mu : 0.0) : 0.0;
  }
  // Qu = r + B'p, Qx = q + A'p (a lane's columns: coalesced rows of B and A)
  for (int i = tid; i < FB_RIC_NUMAX; i += FB_RIC_THREADS) {
    double s = 0.0;
    if (i < nu) {
      s = g.r ? g.r[m*g.sr + i] : 0.0;
      for (int j = 0; j < ndx; j++) s = fma(B[(long long)j*nu + i], pn[j], s);
    }
    qu[i] = s; dg[i] = 1.0;
  }
  double qx[FB_RIC_NDXMAX/FB_RIC_THREADS];
#pragma unroll
  for (int c = 0; c < FB_RIC_NDXMAX/FB_RIC_THREADS; c++) {
    const int j = tid + FB_RIC_THREADS*c;
    double s = 0.0;
    if (j < ndx) {
      s = g.q ? g.q[m*g.sq + j] : 0.0;
      for (int i = 0; i < ndx; i++) s = fma(A[(long long)i*ndx + j], pn[i], s);
    }
    qx[c] = s;
  }
  // right-looking Cholesky; the diagonal of L keeps the pivots, dg their roots.  Every lane reads the same pivot: the verdict is uniform.
  bool bad = false;
  for (int j = 0; j < nu; j++) {
    __syncthreads();
    const double d = L[j*FB_RIC_LD + j];
    if (!(d > 0.0 && d <= 1.7976931348623157e308)) { bad = true; break; }
    const double s = sqrt(d);
    if (tid == 0) dg[j] = s;
    for (int i = j + 1 + tid; i < nu; i += FB_RIC_THREADS) L[i*FB_RIC_LD + j] /= s;
    __syncthreads();
    const int n = nu - j - 1;
    for (int e = tid; e < n*n; e += FB_RIC_THREADS) {
      const int i = j + 1 + e/n, c = j + 1 + e % n;
      if (c <= i) L[i*FB_RIC_LD + c] = fma(-L[i*FB_RIC_LD + j], L[c*FB_RIC_LD + j], L[i*FB_RIC_LD + c]);
    }
  }
  if (bad) {                                             // failure is data: zero gains for this interval, the nominal is skipped from here on
    for (int e = tid; e < ndx*nu; e += FB_RIC_THREADS) Kt[e] = 0.0;
    if (g.k) for (int i = tid; i < nu; i += FB_RIC_THREADS) g.k[m*g.sk + i] = 0.0;
    if (tid == 0) {
      g.status[m] = 1 + g.t;
      if (g.dV) { g.dV[2*m] = 0.0; g.dV[2*m + 1] = 0.0; }
    }
    return;
  }
  __syncthreads();
  // K = -Quu_reg^-1 Qux and k = -Quu_reg^-1 Qu: column c of Qux (c == ndx: Qu) is one lane's right-hand side, held in registers; the
  // loops are unrolled over FB_RIC_NUMAX with zero rows beyond nu, so every register index is static.
  for (int c = tid; c <= ndx; c += FB_RIC_THREADS) {
    double x[FB_RIC_NUMAX];
#pragma unroll
    for (int i = 0; i < FB_RIC_NUMAX; i++) x[i] = i < nu ? (c < ndx ? Qux[(long long)i*ndx + c] : qu[i]) : 0.0;
#pragma unroll
    for (int i = 0; i < FB_RIC_NUMAX; i++) if (i < nu) {
      double s = x[i];
#pragma unroll
      for (int j = 0; j < i; j++) s = fma(-L[i*FB_RIC_LD + j], x[j], s);
      x[i] = s/dg[i];
    }
#pragma unroll
    for (int i = FB_RIC_NUMAX - 1; i >= 0; i--) if (i < nu) {
      double s = x[i];
#pragma unroll
      for (int j = i + 1; j < FB_RIC_NUMAX; j++) s = fma(-L[j*FB_RIC_LD + i], x[j], s);
      x[i] = s/dg[i];
    }
    if (c < ndx) {
#pragma unroll
      for (int i = 0; i < FB_RIC_NUMAX; i++) if (i < nu) Kt[(long long)c*nu + i] = -x[i];
    }
    else {
#pragma unroll
      for (int i = 0; i < FB_RIC_NUMAX; i++) if (i < nu) { kv[i] = -x[i]; if (g.k) g.k[m*g.sk + i] = -x[i]; }
    }
  }
  __syncthreads();
  // tq = Quu k (without mu), gv = tq + Qu; dV += (2 k'Qu, k'Quu k); p_t = Qx + K'gv + Qux'k
  for (int i = tid; i < nu; i += FB_RIC_THREADS) {
    double s = 0.0;
    for (int j = 0; j < nu; j++) s = fma(Quu[i*nu + j], kv[j], s);
    tq[i] = s; gv[i] = s + qu[i];
  }
  __syncthreads();
  if (tid == 0 && g.dV) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < nu; i++) { a = fma(kv[i], qu[i], a); b = fma(kv[i], tq[i], b); }
    g.dV[2*m] += 2.0*a; g.dV[2*m + 1] += b;
  }
  double* po = g.p_out + m*g.sp_out;
#pragma unroll
  for (int c = 0; c < FB_RIC_NDXMAX/FB_RIC_THREADS; c++) {
    const int j = tid + FB_RIC_THREADS*c;
    if (j < ndx) {
      double s = qx[c];
      for (int i = 0; i < nu; i++) s = fma(Kt[(long long)j*nu + i], gv[i], s);
      for (int i = 0; i < nu; i++) s = fma(Qux[(long long)i*ndx + j], kv[i], s);
      po[j] = s;
    }
  }
}

// P[m] = (S[m] + S[m]')/2.  Grid: n_nom * chunks workgroups.
struct RicSym { const double* S; long long sS; double* P; long long sP; const int* status; int ndx, chunks; };

__global__ void __launch_bounds__(FB_RIC_THREADS) k_riccati_sym(RicSym g) {
  const int m = blockIdx.x/g.chunks, ch = blockIdx.x % g.chunks, n = g.ndx;
  if (g.status[m] != 0) return;
  const double* S = g.S + m*g.sS; double* P = g.P + m*g.sP;
  for (int e = ch*FB_RIC_THREADS + threadIdx.x; e < n*n; e += g.chunks*FB_RIC_THREADS) {
    const int i = e/n, j = e % n;
    P[e] = 0.5*(S[e] + S[(long long)j*n + i]);
  }
}

// The start of the recursion: P_T = Qf, p_T = q_T (NULL: zero), status = 0, dV = 0.  Grid: n_nom * chunks workgroups.
struct RicInit { const double* Qf; double* P; long long sP; const double* qT; long long sqT; double* p; long long sp; double* dV; int* status; int ndx, chunks; };

__global__ void __launch_bounds__(FB_RIC_THREADS) k_riccati_init(RicInit g) {
  const int m = blockIdx.x/g.chunks, ch = blockIdx.x % g.chunks, n = g.ndx;
  double* P = g.P + m*g.sP;
  for (int e = ch*FB_RIC_THREADS + threadIdx.x; e < n*n; e += g.chunks*FB_RIC_THREADS) P[e] = g.Qf[e];
  if (ch == 0) {
    for (int j = threadIdx.x; j < n; j += FB_RIC_THREADS) g.p[m*g.sp + j] = g.qT ? g.qT[m*g.sqT + j] : 0.0;
    if (threadIdx.x == 0) {
      g.status[m] = 0;
      if (g.dV) { g.dV[2*m] = 0.0; g.dV[2*m + 1] = 0.0; }
    }
  }
}
