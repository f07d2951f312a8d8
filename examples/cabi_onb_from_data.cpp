// libplship from plain C++ (no Python, no torch): the orthonormal basis built FROM DATA through the C ABI of
// include/plship.h, where examples/cabi_step.cpp has to make its projection up:
//   points -> pls_kernel_gram (k(Z,Z), k(Z,X)) -> pls_sym_eigh -> threshold and scale -> pls_onb_build_projection -> one
//   pls_onb_step,
// each stage checked against a scalar restatement in this file.
//   build: hipcc -O2 -std=c++17 -I include examples/cabi_onb_from_data.cpp -L projected-langevin-sampling_amd -lplship \
//                -Wl,-rpath,$PWD/projected-langevin-sampling_amd -o /tmp/cabi_onb_from_data
// Reference semantics: basis/orthonormal.py:36-68 (Gram matrices, eigh of k(Z,Z) / M, threshold, scaled eigenvectors),
// :98-108 and :128-159 (the step), costs/gaussian.py:86-88.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "plship.h"

#define HIP_OK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return 2;                                                                    \
    }                                                                              \
  } while (0)
#define PLS_OK_(x)                                                                 \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ != 0) {                                                                \
      std::fprintf(stderr, "libplship error %d: %s (%s:%d)\n", rc_, pls_last_error(), __FILE__, __LINE__); \
      return 3;                                                                    \
    }                                                                              \
  } while (0)

template <class T>
static T *to_device(const std::vector<T> &h) {
  T *d = nullptr;
  if (hipMalloc(&d, h.size() * sizeof(T)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}

int main() {
  const int64_t n = 250, m = 70, j = 19, d = 2;  // m > 64: the blocked route of the solver; ragged on purpose
  const double eta = 1e-3, sigma2 = 0.3, threshold = 1e-9, outputscale = 1.3;
  std::mt19937_64 gen(3);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<double> X(n * d), Z(m * d), ls = {0.7, 0.9}, y(n), xi, U;
  for (auto &v : X) v = nd(gen);
  for (int64_t a = 0; a < m; ++a)
    for (int64_t k = 0; k < d; ++k) Z[a * d + k] = X[(3 * a) * d + k];  // inducing points: every third data point
  for (auto &v : y) v = nd(gen);

  double *dX = to_device(X), *dZ = to_device(Z), *dls = to_device(ls), *dy = to_device(y);
  double *dKzz, *dKzx, *dlam, *dV;
  HIP_OK(hipMalloc(&dKzz, m * m * sizeof(double)));
  HIP_OK(hipMalloc(&dKzx, m * n * sizeof(double)));
  HIP_OK(hipMalloc(&dlam, m * sizeof(double)));
  HIP_OK(hipMalloc(&dV, m * m * sizeof(double)));
  if (!dX || !dZ || !dls || !dy) return 2;
  hipStream_t st;
  HIP_OK(hipStreamCreate(&st));

  // k(Z,Z), k(Z,X) (orthonormal.py:36-41) and the eigendecomposition of k(Z,Z) (:46-48; the 1 / M goes onto the eigenvalues)
  PLS_OK_(pls_kernel_gram(PLS_KERNEL_RBF_ARD, dZ, m, dZ, m, d, dls, outputscale, dKzz, m, st));
  PLS_OK_(pls_kernel_gram(PLS_KERNEL_RBF_ARD, dZ, m, dX, n, d, dls, outputscale, dKzx, n, st));
  const size_t eigh_bytes = pls_sym_eigh_workspace_bytes(m);
  void *eigh_ws = nullptr;
  HIP_OK(hipMalloc(&eigh_ws, eigh_bytes));
  int32_t info = -1;
  PLS_OK_(pls_sym_eigh(dKzz, m, m, dlam, dV, m, &info, eigh_ws, eigh_bytes, st));
  HIP_OK(hipStreamSynchronize(st));
  std::vector<double> K(m * m), Kzx(m * n), lam(m), V(m * m);
  HIP_OK(hipMemcpy(K.data(), dKzz, K.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(Kzx.data(), dKzx, Kzx.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lam.data(), dlam, lam.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(V.data(), dV, V.size() * sizeof(double), hipMemcpyDeviceToHost));

  // scalar restatement of the Gram matrix and the defining properties of the decomposition
  auto rbf = [&](const double *a, const double *b) {
    double r2 = 0.0;
    for (int64_t k = 0; k < d; ++k) r2 += (a[k] - b[k]) / ls[k] * ((a[k] - b[k]) / ls[k]);
    return outputscale * std::exp(-0.5 * r2);
  };
  double gram_err = 0.0, res = 0.0, orth = 0.0, lam_max = 0.0;
  for (int64_t a = 0; a < m; ++a) {
    for (int64_t b = 0; b < m; ++b) gram_err = std::fmax(gram_err, std::abs(K[a * m + b] - rbf(&Z[a * d], &Z[b * d])));
    for (int64_t i = 0; i < n; ++i) gram_err = std::fmax(gram_err, std::abs(Kzx[a * n + i] - rbf(&Z[a * d], &X[i * d])));
  }
  for (int64_t k = 0; k < m; ++k) {
    lam_max = std::fmax(lam_max, std::abs(lam[k]));
    if (k && lam[k] < lam[k - 1]) {
      std::fprintf(stderr, "eigenvalues not ascending\n");
      return 4;
    }
    for (int64_t a = 0; a < m; ++a) {
      double kv = 0.0, vv = 0.0;
      for (int64_t b = 0; b < m; ++b) kv += K[a * m + b] * V[b * m + k], vv += V[b * m + a] * V[b * m + k];
      res = std::fmax(res, std::abs(kv - V[a * m + k] * lam[k]));
      orth = std::fmax(orth, std::abs(vv - (a == k ? 1.0 : 0.0)));
    }
  }
  std::printf("gram: max abs err %.2e\n", gram_err);
  std::printf("eigh: info %d, max|K V - V L| / ||K||_2 = %.2e, max|V^T V - I| = %.2e\n", (int)info, res / lam_max, orth);
  if (info != 0 || !(gram_err < 1e-13) || !(res / lam_max < 1e-13) || !(orth < 1e-13)) {
    std::fprintf(stderr, "gram / eigh failure\n");
    return 4;
  }

  // threshold and scale (orthonormal.py:52-68): keep lam / M > threshold, Vs = V[:, kept] / sqrt(Mk lam / M)
  std::vector<int64_t> kept;
  for (int64_t k = 0; k < m; ++k)
    if (lam[k] / m > threshold) kept.push_back(k);
  const int64_t mk = (int64_t)kept.size();
  std::printf("kept %lld of %lld eigenvalues\n", (long long)mk, (long long)m);
  if (mk < 2) return 5;
  std::vector<double> Vs(m * mk), lamk(mk);
  for (int64_t c = 0; c < mk; ++c) {
    lamk[c] = lam[kept[c]] / m;
    for (int64_t a = 0; a < m; ++a) Vs[a * mk + c] = V[a * m + kept[c]] / std::sqrt(mk * lamk[c]);
  }
  double *dVs = to_device(Vs), *dlamk = to_device(lamk), *dA, *dAt, *dout;
  HIP_OK(hipMalloc(&dA, mk * n * sizeof(double)));
  HIP_OK(hipMalloc(&dAt, n * mk * sizeof(double)));
  HIP_OK(hipMalloc(&dout, mk * j * sizeof(double)));
  if (!dVs || !dlamk) return 2;
  PLS_OK_(pls_onb_build_projection(dVs, mk, dKzx, n, m, mk, n, dA, n, dAt, mk, st));

  // one Langevin step on the basis just built, against the scalar loop (A = Vs^T k(Z,X) restated from the host copies)
  U.resize(mk * j), xi.resize(mk * j);
  for (auto &v : U) v = nd(gen);
  for (auto &v : xi) v = nd(gen);
  double *dU = to_device(U), *dxi = to_device(xi);
  if (!dU || !dxi) return 2;
  pls_onb_desc basis{};
  basis.mk = mk, basis.n = n, basis.A = dA, basis.lda = n, basis.At = dAt, basis.ldat = mk, basis.lam = dlamk;
  pls_noise_desc noise{};
  noise.kind = PLS_NOISE_INJECTED, noise.xi = dxi, noise.ldxi = j;
  pls_cost_desc cost{};
  cost.cost = PLS_COST_GAUSSIAN, cost.link = PLS_LINK_IDENTITY, cost.deriv_mode = PLS_DERIV_REFERENCE, cost.p[0] = sigma2;
  cost.jitter = 1e-10;
  const size_t ws_bytes = pls_onb_step_workspace_bytes(&basis, j, n);
  void *ws = nullptr;
  HIP_OK(hipMalloc(&ws, ws_bytes ? ws_bytes : 8));
  PLS_OK_(pls_onb_step(&basis, &cost, dy, dU, j, j, eta, &noise, dout, j, /*out_mode=*/0, /*force_generic=*/1, nullptr, ws, ws_bytes, st));
  HIP_OK(hipStreamSynchronize(st));
  std::vector<double> got(mk * j), A(mk * n);
  HIP_OK(hipMemcpy(got.data(), dout, got.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < mk; ++c)
    for (int64_t i = 0; i < n; ++i) {
      double acc = 0.0;
      for (int64_t a = 0; a < m; ++a) acc += Vs[a * mk + c] * Kzx[a * n + i];
      A[c * n + i] = acc;
    }
  double err = 0.0, scale = 0.0;
  for (int64_t c = 0; c < j; ++c) {
    std::vector<double> G(n);
    for (int64_t i = 0; i < n; ++i) {
      double f = 0.0;
      for (int64_t k = 0; k < mk; ++k) f += A[k * n + i] * U[k * j + c];
      G[i] = (f - y[i]) / sigma2;
    }
    for (int64_t k = 0; k < mk; ++k) {
      double dsum = 0.0;
      for (int64_t i = 0; i < n; ++i) dsum += A[k * n + i] * G[i];
      const double want = -eta * dsum - eta * U[k * j + c] / lamk[k] + std::sqrt(2.0 * eta) * xi[k * j + c];
      err = std::fmax(err, std::abs(got[k * j + c] - want));
      scale = std::fmax(scale, std::abs(want));
    }
  }
  std::printf("step on the basis built from data: max rel err %.2e\n", err / scale);
  if (!(err / scale < 1e-9)) {
    std::fprintf(stderr, "parity failure: %.3e\n", err / scale);
    return 1;
  }
  std::printf("cabi_onb_from_data OK\n");
  return 0;
}
