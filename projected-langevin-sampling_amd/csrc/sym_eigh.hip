// The library's own symmetric eigensolver: two-sided cyclic Jacobi, blocked.
//   jacobi_block_kernel   one workgroup diagonalises one problem of order <= 64 in LDS (the whole solve for m <= 64)
//   rotate_tiles_kernel   W[IJ, KL] <- Q_IJ^T W[IJ, KL] Q_KL and V[:, IJ] <- V[:, IJ] Q_IJ on v_mfma_f64_16x16x4
//   eigh_finish_kernel    ascending order by counting ranks, column permutation, the sign rule of canonicalise_signs
// Replaces torch.linalg.eigh at orthonormal.py:46-48 and samplers.py:27 of the reference.  Every loop on the device has
// a fixed bound and no workgroup waits on another one; the host reads one rotation counter per outer sweep.
#include "sym_eigh.h"

#include <cfloat>
#include <cmath>

#include "gemm_tn_f64.h"  // double4_t and the fragment conventions of v_mfma_f64_16x16x4 (its header comment)

namespace plship {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// scale of the matrix and the non-finite check: one workgroup, two passes over the lower triangle in a fixed order.
// stats[0] = max |a|, stats[1] = sum over the WHOLE symmetric matrix of (a / max)^2, stats[2] = 1 if an entry is not finite
// ---------------------------------------------------------------------------------------------------------------
constexpr int EIGH_NORM_THREADS = 1024;

__device__ inline double block_reduce(double v, double *red, bool take_max) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = EIGH_NORM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = take_max ? fmax(red[tid], red[tid + s]) : red[tid] + red[tid + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(EIGH_NORM_THREADS) void eigh_norm_kernel(const double *A, int64_t lda, int m, double *stats) {
  __shared__ double red[EIGH_NORM_THREADS];
  const int tid = threadIdx.x;
  double amax = 0.0, bad = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = tid; j <= i; j += EIGH_NORM_THREADS) {
      const double a = fabs(A[(int64_t)i * lda + j]);
      if (!(a <= DBL_MAX)) bad = 1.0;  // (NaN or infinity)
      else amax = fmax(amax, a);
    }
  amax = block_reduce(amax, red, true);
  bad = block_reduce(bad, red, true);
  double ssq = 0.0;
  if (amax > 0.0 && bad == 0.0) {
    for (int i = 0; i < m; ++i)
      for (int j = tid; j <= i; j += EIGH_NORM_THREADS) {
        const double a = A[(int64_t)i * lda + j] / amax;
        ssq += (j < i ? 2.0 : 1.0) * a * a;
      }
  }
  ssq = block_reduce(ssq, red, false);
  if (tid == 0) stats[0] = amax, stats[1] = ssq, stats[2] = bad, stats[3] = 0.0;
}

// W <- the symmetric matrix of A's lower triangle, zero-padded to mp; V <- I  (blocked route)
__global__ __launch_bounds__(256) void eigh_init_kernel(const double *A, int64_t lda, int m, int mp, double *W, double *V) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)mp * mp) return;
  const int i = (int)(idx / mp), j = (int)(idx % mp);
  const int hi = i > j ? i : j, lo = i > j ? j : i;
  W[idx] = hi < m ? A[(int64_t)hi * lda + lo] : 0.0;
  V[idx] = i == j ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------
// jacobi_block_kernel.  S (the problem) and QT (the accumulated rotation, transposed: a column rotation of Q walks two
// LDS rows) live in LDS.  A sweep is ne - 1 rounds of ne / 2 disjoint pairs (round_robin_pair); the rotations of a round
// are computed by ne / 2 threads, then every 2 x 2 block S[{p,q},{r,s}] <- J_pq^T S[{p,q},{r,s}] J_rs is updated by one
// thread, which also writes the mirrored block, so S stays symmetric to the bit.  A pair rotates only when
// |s_pq| > thr (absolute, passed in); rows and columns of zeros (an odd order's dummy, the padding of the blocked
// route) therefore never rotate and stay zero: c * 0 - s * 0.
//   BLOCKED = false: the problem is the lower triangle of src (order n <= 64); Q goes to Qout (n x n, pitch 64), the
//                    diagonal to Sout, and *not_converged says whether the last sweep still rotated.
//   BLOCKED = true:  workgroup k takes pair k of `round` among nb blocks of 32 of W = src = Sout (pitch ld; n = the order
//                    m of the matrix inside W); a block
//                    that meets the dummy has a bye and is diagonalised alone.  Q goes to Qout + 4096 k and the
//                    diagonalised S back into W's diagonal tile, so that tile is never recomputed by a product.
// *rotations receives the number of rotations made (one integer atomic per workgroup: order-free).
// ---------------------------------------------------------------------------------------------------------------
constexpr size_t EIGH_JACOBI_LDS = (size_t)2 * EIGH_SUB * EIGH_LD * sizeof(double) + 32 * (3 * sizeof(double) + 3 * sizeof(int));

template <bool BLOCKED>
__global__ __launch_bounds__(EIGH_JACOBI_THREADS) void jacobi_block_kernel(const double *src, int64_t ld, int n, int nb, int round,
                                                                           double thr, double *Qout, double *Sout,
                                                                           int *rotations, int *not_converged) {
  extern __shared__ double eigh_lds[];
  double *Sm = eigh_lds, *QT = Sm + EIGH_SUB * EIGH_LD;
  double *pc = QT + EIGH_SUB * EIGH_LD, *ps = pc + 32, *pt = ps + 32;
  int *pp = reinterpret_cast<int *>(pt + 32), *pq = pp + 32, *prot = pq + 32;
  const int tid = threadIdx.x;
  int bI = 0, bJ = -1;
  if (BLOCKED) {
    round_robin_pair(eigh_players(nb), round, blockIdx.x, &bI, &bJ);
    if (bJ >= nb) bJ = -1;
  }
  const int ne = BLOCKED ? EIGH_SUB : n + (n & 1), np = ne / 2;
  auto global_index = [&](int i) -> int {
    if (BLOCKED) {
      const int blk = i < EIGH_BLOCK ? bI : bJ;
      return blk < 0 ? -1 : blk * EIGH_BLOCK + (i & (EIGH_BLOCK - 1));
    }
    return i < n ? i : -1;
  };
  for (int idx = tid; idx < EIGH_SUB * EIGH_SUB; idx += EIGH_JACOBI_THREADS)  // (all of it: the polish below runs on 64 x 64)
    QT[(idx >> 6) * EIGH_LD + (idx & 63)] = (idx >> 6) == (idx & 63) ? 1.0 : 0.0;
  for (int idx = tid; idx < ne * ne; idx += EIGH_JACOBI_THREADS) {
    const int i = idx / ne, j = idx - i * ne;
    if (j <= i) {  // the lower triangle, mirrored (global_index is increasing: bI < bJ)
      const int gi = global_index(i), gj = global_index(j);
      const double v = (gi < 0 || gj < 0) ? 0.0 : src[(int64_t)gi * ld + gj];
      Sm[i * EIGH_LD + j] = v;
      Sm[j * EIGH_LD + i] = v;
    }
  }
  __syncthreads();

  int total = 0, last = 0;
  for (int sweep = 0; sweep < EIGH_INNER_SWEEPS; ++sweep) {
    int swept = 0;
    for (int r = 0; r < ne - 1; ++r) {
      int rot = 0;
      if (tid < np) {
        int p, q;
        round_robin_pair(ne, r, tid, &p, &q);
        const double app = Sm[p * EIGH_LD + p], aqq = Sm[q * EIGH_LD + q], apq = Sm[q * EIGH_LD + p];
        double c = 1.0, s = 0.0, t = 0.0;
        if (fabs(apq) > thr) {
          // t = sign(tau) / (|tau| + hypot(1, tau)): the smaller root, |t| <= 1; hypot without forming tau^2 when it is large
          const double tau = 0.5 * (aqq - app) / apq, at = fabs(tau);
          const double h = at > 1.0 ? at * sqrt(1.0 + (1.0 / at) * (1.0 / at)) : sqrt(1.0 + at * at);
          t = copysign(1.0 / (at + h), tau);
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
          rot = 1;
        }
        pc[tid] = c, ps[tid] = s, pt[tid] = t, pp[tid] = p, pq[tid] = q, prot[tid] = rot;
      }
      const int cnt = __syncthreads_count(rot);
      if (cnt == 0) continue;  // (uniform) nothing to apply; the parameter slots are not read before they are rewritten
      swept += cnt;
      for (int idx = tid; idx < np * np; idx += EIGH_JACOBI_THREADS) {
        const int a = idx / np, b = idx - a * np;
        if (a > b || !(prot[a] | prot[b])) continue;
        const int p = pp[a], q = pq[a];
        if (a == b) {  // the pivot block: the off-diagonal entry is annihilated exactly
          const double apq = Sm[q * EIGH_LD + p], t = pt[a];
          Sm[p * EIGH_LD + p] -= t * apq;
          Sm[q * EIGH_LD + q] += t * apq;
          Sm[p * EIGH_LD + q] = 0.0;
          Sm[q * EIGH_LD + p] = 0.0;
          continue;
        }
        const int u = pp[b], v = pq[b];
        const double c1 = pc[a], s1 = ps[a], c2 = pc[b], s2 = ps[b];
        const double xpu = Sm[p * EIGH_LD + u], xpv = Sm[p * EIGH_LD + v], xqu = Sm[q * EIGH_LD + u], xqv = Sm[q * EIGH_LD + v];
        // rows first (J_pq^T .), then columns (. J_uv): a fixed order
        const double ypu = c1 * xpu - s1 * xqu, ypv = c1 * xpv - s1 * xqv;
        const double yqu = s1 * xpu + c1 * xqu, yqv = s1 * xpv + c1 * xqv;
        const double zpu = c2 * ypu - s2 * ypv, zpv = s2 * ypu + c2 * ypv;
        const double zqu = c2 * yqu - s2 * yqv, zqv = s2 * yqu + c2 * yqv;
        Sm[p * EIGH_LD + u] = zpu, Sm[u * EIGH_LD + p] = zpu;
        Sm[p * EIGH_LD + v] = zpv, Sm[v * EIGH_LD + p] = zpv;
        Sm[q * EIGH_LD + u] = zqu, Sm[u * EIGH_LD + q] = zqu;
        Sm[q * EIGH_LD + v] = zqv, Sm[v * EIGH_LD + q] = zqv;
      }
      for (int idx = tid; idx < np * ne; idx += EIGH_JACOBI_THREADS) {  // Q <- Q J: rows p, q of QT
        const int b = idx / ne, i = idx - b * ne;
        if (!prot[b]) continue;
        const double c = pc[b], s = ps[b];
        const double xp = QT[pp[b] * EIGH_LD + i], xq = QT[pq[b] * EIGH_LD + i];
        QT[pp[b] * EIGH_LD + i] = c * xp - s * xq;
        QT[pq[b] * EIGH_LD + i] = s * xp + c * xq;
      }
      __syncthreads();
    }
    last = swept;
    total += swept;
    if (swept == 0) break;
  }

  double *Q = Qout + (BLOCKED ? (int64_t)blockIdx.x * EIGH_SUB * EIGH_SUB : 0);
  const int nq = BLOCKED ? EIGH_SUB : n;
  // BLOCKED: the pair's eigenvalues leave in descending |.| (ties: the smaller index first), a column permutation of Q,
  // so that large eigenvalues gather in the leading blocks and the working matrix becomes graded IN ORDER; without it
  // a spectrum that spans 17 decades (an RBF Gram matrix) gains less than a decade per outer sweep.  Only live indices
  // (inside the matrix, below n = m) are permuted: the padding keeps its place.
  int *dest = pp, *slot = reinterpret_cast<int *>(pc);  // 64 ints each (pp and pq; pc)
  if (BLOCKED) {
    int rank = 0, ordinal = 0;
    bool live = false;
    if (tid < EIGH_SUB) {
      const int gi = global_index(tid);
      live = gi >= 0 && gi < n;
      const double di = fabs(Sm[tid * EIGH_LD + tid]);
      for (int j = 0; j < EIGH_SUB; ++j) {
        const int gj = global_index(j);
        if (gj < 0 || gj >= n) continue;
        const double dj = fabs(Sm[j * EIGH_LD + j]);
        ordinal += j < tid ? 1 : 0;
        rank += (dj > di || (dj == di && j < tid)) ? 1 : 0;
      }
      if (live) slot[ordinal] = tid;
    }
    __syncthreads();
    if (tid < EIGH_SUB) dest[tid] = live ? slot[rank] : tid;
    __syncthreads();
    for (int idx = tid; idx < nq * nq; idx += EIGH_JACOBI_THREADS) {
      const int i = idx / nq, k = idx - i * nq;
      const int gi = global_index(dest[i]), gk = global_index(dest[k]);
      if (gi >= 0 && gk >= 0) Sout[(int64_t)gi * ld + gk] = Sm[i * EIGH_LD + k];
    }
  } else {
    for (int i = tid; i < n; i += EIGH_JACOBI_THREADS) Sout[i] = Sm[i * EIGH_LD + i];
  }
  // Polish: thousands of rotations leave Q orthogonal to some 100 eps only, and V is a product of many such Q.  One
  // Newton-Schulz step Q <- Q - Q (Q^T Q - I) / 2 brings Q^T Q - I down to the rounding of that product.  With QT = Q^T
  // in LDS: E = QT QT^T - I (into S's place, which is written out by now), then QT <- QT - E QT / 2.  Both products are
  // 64 x 64 x 64 on v_mfma_f64_16x16x4; wave w owns rows 16 (w / 2) .. + 15 and columns 32 (w % 2) .. + 31.  The
  // padding stays untouched: its rows of QT are unit vectors, its rows and columns of E are zero.
  if (total > 0) {  // (uniform; no rotation: Q is the identity to the bit)
    const int lane = tid & 63, wave = tid >> 6, q4 = lane >> 4, c16 = lane & 15;
    const int i0 = 16 * (wave >> 1), j0 = 32 * (wave & 1);
    double4_t acc[2];
    __syncthreads();  // S is written out
    acc[0] = acc[1] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int kq = 0; kq < EIGH_SUB / 4; ++kq) {
      const int k = 4 * kq + q4;
      const double fa = QT[(i0 + c16) * EIGH_LD + k];
      for (int tj = 0; tj < 2; ++tj)
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, QT[(j0 + 16 * tj + c16) * EIGH_LD + k], acc[tj], 0, 0, 0);
    }
    for (int tj = 0; tj < 2; ++tj)
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * r + q4, j = j0 + 16 * tj + c16;
        Sm[i * EIGH_LD + j] = acc[tj][r] - (i == j ? 1.0 : 0.0);
      }
    __syncthreads();
    acc[0] = acc[1] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int kq = 0; kq < EIGH_SUB / 4; ++kq) {
      const int k = 4 * kq + q4;
      const double fa = Sm[(i0 + c16) * EIGH_LD + k];
      for (int tj = 0; tj < 2; ++tj)
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, QT[k * EIGH_LD + j0 + 16 * tj + c16], acc[tj], 0, 0, 0);
    }
    __syncthreads();  // every wave has read QT
    for (int tj = 0; tj < 2; ++tj)
      for (int r = 0; r < 4; ++r) QT[(i0 + 4 * r + q4) * EIGH_LD + j0 + 16 * tj + c16] -= 0.5 * acc[tj][r];
    __syncthreads();
  }
  for (int idx = tid; idx < nq * nq; idx += EIGH_JACOBI_THREADS) {
    const int i = idx / nq, k = idx - i * nq;
    Q[i * EIGH_SUB + (BLOCKED ? dest[k] : k)] = QT[k * EIGH_LD + i];
  }
  if (tid == 0) {
    if (total > 0) atomicAdd(rotations, total);
    if (!BLOCKED) *not_converged = last > 0 ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// rotate_tiles_kernel: one 64 x 64 tile per workgroup, T = [Q_a^T] X Q_b with the operands staged in LDS and the products
// on v_mfma_f64_16x16x4 (lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; the result sits as
// C[i = (l >> 4) + 4 reg][j = l & 15]; accumulators stay in place).  Wave w owns rows 16 w .. 16 w + 15 of the tile.
//   TWO_SIDED: tile (a, b), a < b, of the working matrix W: rows = blocks of pair a, columns = blocks of pair b of
//              `round`; T goes to W[a, b] and T^T to W[b, a], so W stays symmetric to the bit and the grid's other half
//              (a >= b; the diagonal tiles were written by jacobi_block_kernel) returns at once.
//   otherwise: rows 64 c .. 64 c + 63 of V, columns = blocks of pair b: V[:, IJ] <- V[:, IJ] Q_IJ.
// A block index beyond nb (the dummy of an odd count, the ragged last row chunk) reads zeros and stores nothing.
// Every tile is read and written by exactly one workgroup: in place, no atomics.
// ---------------------------------------------------------------------------------------------------------------
constexpr size_t EIGH_TILE_LDS = (size_t)3 * EIGH_SUB * EIGH_LD * sizeof(double);

template <bool TWO_SIDED>
__global__ __launch_bounds__(EIGH_TILE_THREADS) void rotate_tiles_kernel(double *M, int64_t ld, const double *Q, int nb, int round) {
  extern __shared__ double eigh_lds[];
  double *X = eigh_lds, *QA = X + EIGH_SUB * EIGH_LD, *QB = QA + EIGH_SUB * EIGH_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int players = eigh_players(nb);
  const int a = blockIdx.x, b = blockIdx.y;
  int rb[2], cb[2];
  if (TWO_SIDED) {
    if (a >= b) return;
    round_robin_pair(players, round, a, &rb[0], &rb[1]);
  } else {
    rb[0] = 2 * a, rb[1] = 2 * a + 1;
  }
  round_robin_pair(players, round, b, &cb[0], &cb[1]);
  for (int h = 0; h < 2; ++h) {
    if (rb[h] >= nb) rb[h] = -1;
    if (cb[h] >= nb) cb[h] = -1;
  }
  auto row_of = [&](int i) { const int blk = rb[i >> 5]; return blk < 0 ? -1 : blk * EIGH_BLOCK + (i & 31); };
  auto col_of = [&](int j) { const int blk = cb[j >> 5]; return blk < 0 ? -1 : blk * EIGH_BLOCK + (j & 31); };

  const double *Qa = Q + (int64_t)a * EIGH_SUB * EIGH_SUB, *Qb = Q + (int64_t)b * EIGH_SUB * EIGH_SUB;
  for (int idx = tid; idx < EIGH_SUB * EIGH_SUB; idx += EIGH_TILE_THREADS) {
    const int i = idx >> 6, j = idx & 63;
    const int gi = row_of(i), gj = col_of(j);
    X[i * EIGH_LD + j] = (gi < 0 || gj < 0) ? 0.0 : M[(int64_t)gi * ld + gj];
    QB[i * EIGH_LD + j] = Qb[idx];
    if (TWO_SIDED) QA[i * EIGH_LD + j] = Qa[idx];
  }
  __syncthreads();

  const int q4 = lane >> 4, c16 = lane & 15, i0 = 16 * wave;
  double4_t acc[4];
  if (TWO_SIDED) {  // Y = Q_a^T X, written over X
    for (int tj = 0; tj < 4; ++tj) acc[tj] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int kq = 0; kq < EIGH_SUB / 4; ++kq) {
      const int k = 4 * kq + q4;
      const double fa = QA[k * EIGH_LD + i0 + c16];
      for (int tj = 0; tj < 4; ++tj)
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, X[k * EIGH_LD + 16 * tj + c16], acc[tj], 0, 0, 0);
    }
    __syncthreads();
    for (int tj = 0; tj < 4; ++tj)
      for (int r = 0; r < 4; ++r) X[(i0 + 4 * r + q4) * EIGH_LD + 16 * tj + c16] = acc[tj][r];
    __syncthreads();
  }
  for (int tj = 0; tj < 4; ++tj) acc[tj] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int kq = 0; kq < EIGH_SUB / 4; ++kq) {  // T = X Q_b
    const int k = 4 * kq + q4;
    const double fa = X[(i0 + c16) * EIGH_LD + k];
    for (int tj = 0; tj < 4; ++tj)
      acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, QB[k * EIGH_LD + 16 * tj + c16], acc[tj], 0, 0, 0);
  }
  __syncthreads();
  for (int tj = 0; tj < 4; ++tj)
    for (int r = 0; r < 4; ++r) X[(i0 + 4 * r + q4) * EIGH_LD + 16 * tj + c16] = acc[tj][r];
  __syncthreads();
  for (int idx = tid; idx < EIGH_SUB * EIGH_SUB; idx += EIGH_TILE_THREADS) {
    const int i = idx >> 6, j = idx & 63;
    const int gi = row_of(i), gj = col_of(j);
    if (gi >= 0 && gj >= 0) M[(int64_t)gi * ld + gj] = X[i * EIGH_LD + j];
    if (TWO_SIDED) {  // the mirrored tile: row col_of(i), column row_of(j) <- T[j][i]
      const int hi = col_of(i), hj = row_of(j);
      if (hi >= 0 && hj >= 0) M[(int64_t)hi * ld + hj] = X[j * EIGH_LD + i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// eigh_finish_kernel: workgroup i takes the i-th diagonal entry d_i and column i of Vw.  Its place in the ascending order
// is the number of entries that are smaller, or equal with a smaller index; the column's largest-magnitude component
// (the first one on ties) is made positive -- canonicalise_signs of basis/spectrum.py.  Only the first m rows, columns
// and diagonal entries are looked at: the padding is dropped here.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eigh_finish_kernel(const double *d, int64_t dstride, const double *Vw, int64_t ldvw, int m,
                                                          double *lam, double *V, int64_t ldv) {
  __shared__ int s_rank;
  __shared__ double s_abs[256];
  __shared__ int s_idx[256];
  const int tid = threadIdx.x, i = blockIdx.x;
  if (tid == 0) s_rank = 0;
  __syncthreads();
  const double di = d[(int64_t)i * dstride];
  int count = 0;
  for (int j = tid; j < m; j += 256) {
    const double dj = d[(int64_t)j * dstride];
    count += (dj < di || (dj == di && j < i)) ? 1 : 0;
  }
  if (count) atomicAdd(&s_rank, count);
  double best = -1.0;
  int arg = 0;
  for (int r = tid; r < m; r += 256) {
    const double v = fabs(Vw[(int64_t)r * ldvw + i]);
    if (v > best) best = v, arg = r;
  }
  s_abs[tid] = best, s_idx[tid] = arg;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const double o = s_abs[tid + s];
      const int oi = s_idx[tid + s];
      if (o > s_abs[tid] || (o == s_abs[tid] && oi < s_idx[tid])) s_abs[tid] = o, s_idx[tid] = oi;
    }
    __syncthreads();
  }
  const int rank = s_rank;
  const double sign = Vw[(int64_t)s_idx[0] * ldvw + i] < 0.0 ? -1.0 : 1.0;
  if (tid == 0) lam[rank] = di;
  for (int r = tid; r < m; r += 256) V[(int64_t)r * ldv + rank] = sign * Vw[(int64_t)r * ldvw + i];
}

// ---------------------------------------------------------------------------------------------------------------
// launchers: one per kernel, holding grid, LDS size, timeline tag and check_launch name
// ---------------------------------------------------------------------------------------------------------------
int launch_norm(const double *A, int64_t lda, int m, double *stats, hipStream_t st) {
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(eigh_norm_kernel, dim3(1), dim3(EIGH_NORM_THREADS), 0, st, A, lda, m, stats);
  }
  return check_launch("eigh_norm");
}

int launch_init(const double *A, int64_t lda, int m, int mp, double *W, double *V, hipStream_t st) {
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(eigh_init_kernel, dim3((unsigned)cdiv((int64_t)mp * mp, 256)), dim3(256), 0, st, A, lda, m, mp, W, V);
  }
  return check_launch("eigh_init");
}

template <bool BLOCKED>
int launch_jacobi(int problems, const double *src, int64_t ld, int n, int nb, int round, double thr, double *Qout, double *Sout,
                  int *rotations, int *not_converged, hipStream_t st) {
  if (int rc = ensure_lds<jacobi_block_kernel<BLOCKED>>(EIGH_JACOBI_LDS)) return rc;
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL((jacobi_block_kernel<BLOCKED>), dim3(problems), dim3(EIGH_JACOBI_THREADS), EIGH_JACOBI_LDS, st, src, ld, n, nb,
                       round, thr, Qout, Sout, rotations, not_converged);
  }
  return check_launch("jacobi_block");
}

template <bool TWO_SIDED>
int launch_rotate_tiles(int rows, int pairs, double *M, int64_t ld, const double *Q, int nb, int round, hipStream_t st) {
  if (int rc = ensure_lds<rotate_tiles_kernel<TWO_SIDED>>(EIGH_TILE_LDS)) return rc;
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL((rotate_tiles_kernel<TWO_SIDED>), dim3(rows, pairs), dim3(EIGH_TILE_THREADS), EIGH_TILE_LDS, st, M, ld, Q, nb,
                       round);
  }
  return check_launch("rotate_tiles");
}

int launch_finish(const double *d, int64_t dstride, const double *Vw, int64_t ldvw, int m, double *lam, double *V, int64_t ldv,
                  hipStream_t st) {
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(eigh_finish_kernel, dim3(m), dim3(256), 0, st, d, dstride, Vw, ldvw, m, lam, V, ldv);
  }
  return check_launch("eigh_finish");
}

// the pinned words the host reads after a synchronisation: allocated once per calling thread, never inside a sweep
struct PinnedWords {  // (64 bytes per calling thread, kept for the life of the process: no HIP call in a thread's teardown)
  double *p = nullptr;
};

int pinned_words(double **out) {
  static thread_local PinnedWords words;
  if (!words.p) {
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&words.p), 8 * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) return fail(PLS_ERR_HIP, "pls_sym_eigh: hipHostMalloc: %s", hipGetErrorString(e));
  }
  *out = words.p;
  return PLS_OK;
}

int read_back(void *host, const void *dev, size_t bytes, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(PLS_ERR_HIP, "pls_sym_eigh: read-back: %s", hipGetErrorString(e));
  return PLS_OK;
}

}  // namespace
}  // namespace plship

using namespace plship;

extern "C" {

size_t pls_sym_eigh_workspace_bytes(int64_t m) { return (size_t)eigh_layout(m).total * sizeof(double); }

int64_t pls_sym_eigh_round_pairs(int64_t nblocks, int64_t round, int64_t *pairs) {
  if (nblocks < 2 || !pairs) return 0;
  const int players = eigh_players(nblocks);
  if (round < 0 || round >= players - 1) return 0;
  int64_t count = 0;
  for (int k = 0; k < players / 2; ++k) {
    int lo, hi;
    round_robin_pair(players, (int)round, k, &lo, &hi);
    if (hi >= nblocks) continue;  // the dummy: lo has a bye
    pairs[2 * count] = lo, pairs[2 * count + 1] = hi;
    ++count;
  }
  return count;
}

int pls_sym_eigh(const double *A, int64_t lda, int64_t m, double *lam, double *V, int64_t ldv, int32_t *info, void *ws,
                 size_t ws_bytes, void *stream) {
  PLS_REQUIRE(m >= 0, "pls_sym_eigh: m = %lld < 0", (long long)m);
  if (m == 0) return PLS_OK;
  PLS_REQUIRE(A && lam && V && info, "pls_sym_eigh: NULL argument (A, lam, V and info are required)");
  PLS_REQUIRE(lda >= m, "pls_sym_eigh: lda = %lld < m = %lld", (long long)lda, (long long)m);
  PLS_REQUIRE(ldv >= m, "pls_sym_eigh: ldv = %lld < m = %lld", (long long)ldv, (long long)m);
  PLS_REQUIRE(m <= (int64_t)1 << 15, "pls_sym_eigh: m = %lld is beyond 32768", (long long)m);
  const EighLayout l = eigh_layout(m);
  PLS_REQUIRE(ws != nullptr, "pls_sym_eigh: NULL workspace");
  PLS_REQUIRE(ws_bytes >= (size_t)l.total * sizeof(double), "pls_sym_eigh: workspace of %zu bytes, pls_sym_eigh_workspace_bytes(%lld) = %zu",
              ws_bytes, (long long)m, (size_t)l.total * sizeof(double));
  PLS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "pls_sym_eigh: the workspace must be 8-byte aligned");
  hipStream_t st = S(stream);
  double *base = static_cast<double *>(ws);
  double *W = base + l.w, *Vw = base + l.v, *Q = base + l.q, *stats = base + l.stats;
  int *counters = reinterpret_cast<int *>(base + l.counters);
  double *pinned = nullptr;
  if (int rc = pinned_words(&pinned)) return rc;

  if (hipMemsetAsync(counters, 0, (EIGH_OUTER_SWEEPS + 2) * sizeof(int), st) != hipSuccess)
    return fail(PLS_ERR_HIP, "pls_sym_eigh: hipMemsetAsync failed");
  if (int rc = launch_norm(A, lda, (int)m, stats, st)) return rc;
  if (int rc = read_back(pinned, stats, 4 * sizeof(double), st)) return rc;
  if (pinned[2] != 0.0) return fail(PLS_ERR_INVALID_ARGUMENT, "pls_sym_eigh: non-finite entry in the lower triangle of A");
  // |s_pq| <= thr = eps ||A||_F / m ends the rotations of a pair: absolute, so rounding-level eigenvalues settle
  const double thr = DBL_EPSILON * (pinned[0] * std::sqrt(pinned[1])) / (double)m;

  if (l.nb == 0) {
    int *flag = counters + EIGH_OUTER_SWEEPS;
    if (int rc = launch_jacobi<false>(1, A, lda, (int)m, 0, 0, thr, Vw, W, counters, flag, st)) return rc;
    if (int rc = launch_finish(W, 1, Vw, EIGH_SUB, (int)m, lam, V, ldv, st)) return rc;
    int *host_flag = reinterpret_cast<int *>(pinned);
    if (int rc = read_back(host_flag, flag, sizeof(int), st)) return rc;
    *info = *host_flag ? 1 : 0;
    return PLS_OK;
  }

  const int nb = (int)l.nb, mp = (int)l.mp, players = eigh_players(nb), pairs = players / 2;
  if (int rc = launch_init(A, lda, (int)m, mp, W, Vw, st)) return rc;
  int32_t not_converged = 1;
  for (int sweep = 0; sweep < EIGH_OUTER_SWEEPS; ++sweep) {
    for (int round = 0; round < players - 1; ++round) {
      if (int rc = launch_jacobi<true>(pairs, W, mp, (int)m, nb, round, thr, Q, W, counters + sweep, nullptr, st)) return rc;
      if (int rc = launch_rotate_tiles<true>(pairs, pairs, W, mp, Q, nb, round, st)) return rc;
      if (int rc = launch_rotate_tiles<false>((int)cdiv(nb, 2), pairs, Vw, mp, Q, nb, round, st)) return rc;
    }
    int *host_count = reinterpret_cast<int *>(pinned);
    if (int rc = read_back(host_count, counters + sweep, sizeof(int), st)) return rc;
    if (*host_count == 0) {
      not_converged = 0;
      break;
    }
  }
  if (int rc = launch_finish(W, (int64_t)mp + 1, Vw, mp, (int)m, lam, V, ldv, st)) return rc;
  *info = not_converged;
  return PLS_OK;
}

}  // extern "C"
