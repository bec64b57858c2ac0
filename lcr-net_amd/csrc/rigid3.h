// rigid3.h — fp64 3x3 rotation fit shared by the weighted Procrustes (lgr.hip), the RANSAC hypotheses (ransac.hip) and the point-to-point
// ICP update (icp.hip), and the fp64 symmetric 3x3 eigen-solver of the surface normals (normals.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace lcr {

// 3x3 SVD by one-sided Jacobi (Hestenes) in fp64: A V = U S.  Returns R = V diag(1,1,sign det(V U^T)) U^T, and the singular values of H
// in decreasing order in sv (rotation_from_H_sv: the RANSAC degeneracy test reads them).
template <bool SV>
__device__ inline void rotation_from_H_impl(const double H[3][3], double R[3][3], double* sv) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = H[i][j];
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int k = 0; k < 3; ++k) {
          alpha += A[k][p] * A[k][p];
          beta += A[k][q] * A[k][q];
          gamma += A[k][p] * A[k][q];
        }
        off = fmax(off, fabs(gamma) / (sqrt(alpha * beta) + 1e-300));
        if (fabs(gamma) < 1e-300) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 3; ++k) {
          const double ap = A[k][p], aq = A[k][q];
          A[k][p] = c * ap - s * aq;
          A[k][q] = s * ap + c * aq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  // singular values = column norms of A; U = A / sigma.  Order columns by decreasing sigma (like LAPACK) so that the
  // reflection fix hits the smallest singular direction.
  double sig[3];
  int ord[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  for (int a = 0; a < 2; ++a)
    for (int b2 = a + 1; b2 < 3; ++b2)
      if (sig[ord[b2]] > sig[ord[a]]) {
        const int tmp = ord[a];
        ord[a] = ord[b2];
        ord[b2] = tmp;
      }
  double U[3][3], Vs[3][3];
  for (int j = 0; j < 3; ++j) {
    const int c = ord[j];
    for (int k = 0; k < 3; ++k) {
      Vs[k][j] = V[k][c];
      U[k][j] = sig[c] > 1e-300 ? A[k][c] / sig[c] : 0.0;
    }
  }
  // H == 0 (no correspondence, or every weight zero): no direction at all.  Start U from the canonical basis; the completion below then
  // gives U = I, and V = I (no rotation was applied) gives R = I exactly, as torch.svd of a zero matrix does.
  if (!(sig[ord[0]] > 1e-300)) U[0][0] = 1.0;
  // complete U if rank deficient: third column = u0 x u1 (and second from any orthogonal vector if needed)
  if (sig[ord[1]] <= 1e-12 * sig[ord[0]] || sig[ord[1]] <= 1e-300) {
    // pick an axis least aligned with u0
    int ax = 0;
    if (fabs(U[1][0]) < fabs(U[ax][0])) ax = 1;
    if (fabs(U[2][0]) < fabs(U[ax][0])) ax = 2;
    double e[3] = {0, 0, 0};
    e[ax] = 1.0;
    const double d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0];
    double nrm = 0;
    for (int k = 0; k < 3; ++k) {
      U[k][1] = e[k] - d * U[k][0];
      nrm += U[k][1] * U[k][1];
    }
    nrm = sqrt(nrm);
    for (int k = 0; k < 3; ++k) U[k][1] /= nrm;
  }
  if (sig[ord[2]] <= 1e-12 * sig[ord[0]] || sig[ord[2]] <= 1e-300) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
  auto det3 = [](const double X[3][3]) {
    return X[0][0] * (X[1][1] * X[2][2] - X[1][2] * X[2][1]) - X[0][1] * (X[1][0] * X[2][2] - X[1][2] * X[2][0]) +
           X[0][2] * (X[1][0] * X[2][1] - X[1][1] * X[2][0]);
  };
  const double sgn = det3(Vs) * det3(U) >= 0 ? 1.0 : -1.0;   // det(V U^T) = det V * det U
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = Vs[i][0] * U[j][0] + Vs[i][1] * U[j][1] + sgn * Vs[i][2] * U[j][2];
  if constexpr (SV)
    for (int j = 0; j < 3; ++j) sv[j] = sig[ord[j]];
}

__device__ inline void rotation_from_H(const double H[3][3], double R[3][3]) { rotation_from_H_impl<false>(H, R, nullptr); }
__device__ inline void rotation_from_H_sv(const double H[3][3], double R[3][3], double sv[3]) { rotation_from_H_impl<true>(H, R, sv); }

// Eigen-decomposition of a symmetric 3x3 matrix by cyclic Jacobi rotations in fp64: A = V diag(lam) V^T with lam ascending and the
// eigenvectors in the columns of V (orthonormal up to rounding).  Sweeps stop once the off-diagonal mass is below 1e-36 of the diagonal's
// (or zero), at most 50.
__device__ inline void sym3_eigen(const double A[3][3], double lam[3], double V[3][3]) {
  double a[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      a[i][j] = A[i][j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (off == 0.0 || off <= 1e-36 * dia) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {             // a <- a J (columns p, q)
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {             // a <- J^T a (rows p, q)
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = a[q][p] = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int ord[3] = {0, 1, 2};
  for (int x = 0; x < 2; ++x)
    for (int y = x + 1; y < 3; ++y)
      if (a[ord[y]][ord[y]] < a[ord[x]][ord[x]]) {
        const int tmp = ord[x];
        ord[x] = ord[y];
        ord[y] = tmp;
      }
  double W[3][3];
  for (int j = 0; j < 3; ++j) {
    lam[j] = a[ord[j]][ord[j]];
    for (int k = 0; k < 3; ++k) W[k][j] = V[k][ord[j]];
  }
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 3; ++j) V[k][j] = W[k][j];
}

}  // namespace lcr
