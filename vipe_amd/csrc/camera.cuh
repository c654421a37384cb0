// Camera models of the dense BA (pinhole, MEI, 360-degree panorama), per-pixel, with the Jacobians the solver needs.
// Restates vipe/utils/cameras.py:131-207 (pinhole) and :228-336 (MEI); MIN_DEPTH = 0.1 (cameras.py:48).
// The panorama follows PanoramaCameraModel.iproj_disp (cameras.py:366-387) and project_points_to_panorama
// (vipe/utils/geometry.py:89-120) on the pixel-centre grid, u_n = (u + 0.5) / wd; the reference has no proj_points for it,
// so its projection Jacobian, validity and seam rules are this project's:
//   ray        theta = ((u + 0.5) / wd - 0.5) 2 pi, phi = (v + 0.5) / ht pi, b = (sin phi sin theta, -cos phi, sin phi cos theta)
//   point      X0 = (b, d) with d the inverse RANGE; X1 = R b + t d
//   projection theta = atan2(X, Z), phi = atan2(rho, -Y), rho = |(X, Z)|, r = |X1|;  x = (theta / 2 pi + 0.5) wd - 0.5 in
//              [-0.5, wd - 0.5), y = phi / pi ht - 0.5
//   validity   r > MIN_DEPTH and rho > POLE_EPS r (no z clamp); every horizontal difference is wrapped into [-wd/2, wd/2)
#pragma once
#include "common.cuh"

namespace cam {

constexpr float MIN_DEPTH = 0.1f;
constexpr float POLE_EPS = 1e-3f;  // panorama: 0.06 degrees off the pole, inside the first row of any grid up to 1500 rows
constexpr float PI_F = 3.14159265358979323846f;

// panorama: there are no intrinsics; the slots carry the grid instead: fx = wd / 2 pi, fy = ht / pi, cx = wd, cy = ht
struct Intr {
  float fx, fy, cx, cy, k1;
};

// intrinsics row [4+D] at full resolution -> scaled by `s` (cameras.py:212-213, :345-348: k1 is not scaled)
__host__ __device__ inline Intr load_scaled(const float* p, int D, float s) {
  Intr I;
  I.fx = p[0] * s;
  I.fy = p[1] * s;
  I.cx = p[2] * s;
  I.cy = p[3] * s;
  I.k1 = D > 0 ? p[4] : 0.0f;
  return I;
}

// what a kernel instantiated for CAM holds of a view: its scaled row, or - panorama - the grid (the row is never read)
template <int CAM>
__host__ __device__ inline Intr load(const float* row, int D, float s, int ht, int wd) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) {
    Intr I;
    I.fx = (float)wd / (2.0f * PI_F);
    I.fy = (float)ht / PI_F;
    I.cx = (float)wd;
    I.cy = (float)ht;
    I.k1 = 0.0f;
    return I;
  } else {
    return load_scaled(row, D, s);
  }
}

// target-side validity of the transformed point (geom.py:263 for pinhole / MEI)
template <int CAM>
__device__ __forceinline__ bool valid_point(float X, float Y, float Z) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) {
    const float rho2 = X * X + Z * Z;
    const float r = sqrtf(rho2 + Y * Y);
    return r > MIN_DEPTH && sqrtf(rho2) > POLE_EPS * r;
  } else {
    return Z > MIN_DEPTH;
  }
}

// a horizontal difference across the seam of the panorama, wrapped into [-wd/2, wd/2); the identity for the other cameras
template <int CAM>
__device__ __forceinline__ float wrap_dx(float dx, float wd) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) return dx - wd * floorf(dx / wd + 0.5f);
  else return dx;
}

// inverse projection: X0 = (X, Y, Z, d) with Z == 1 for pinhole / MEI (not written: their callers use the constant).  dXf[f] = d(X,Y)/d(intrinsic f), f = 0 focal, f = 1 k1 (MEI)
template <int CAM, int F>
__device__ __forceinline__ void iproj(const Intr& I, float u, float v, float& X, float& Y, float& Z,
                                      float (&dX)[F > 0 ? F : 1], float (&dY)[F > 0 ? F : 1]) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) {
    const float theta = ((u + 0.5f) - 0.5f * I.cx) * (2.0f * PI_F / I.cx);
    const float phi = (v + 0.5f) * (PI_F / I.cy);
    const float sp = sinf(phi);
    X = sp * sinf(theta);
    Y = -cosf(phi);
    Z = sp * cosf(theta);
    if constexpr (F > 0) {  // no intrinsics: the rig walk carries zero rows
#pragma unroll
      for (int f = 0; f < F; ++f) dX[f] = dY[f] = 0.0f;
    }
  } else if constexpr (CAM == VIPE_CAM_PINHOLE) {
    X = (u - I.cx) / I.fx;
    Y = (v - I.cy) / I.fy;
    if constexpr (F > 0) {
      dX[0] = -X / I.fx;
      dY[0] = -Y / I.fy;
    }
  } else {
    const float k1 = I.k1;
    const float ub = (u - I.cx) / I.fx, vb = (v - I.cy) / I.fy;
    const float r2 = ub * ub + vb * vb;
    const float q = sqrtf(1.0f + (1.0f - k1 * k1) * r2);
    const float factor = (k1 + q) / (1.0f + r2);
    X = ub * factor / (factor - k1);
    Y = vb * factor / (factor - k1);
    if constexpr (F > 0) {
      const float k2 = k1 * k1, k3 = k2 * k1, q2 = q * q, r4 = r2 * r2;
      const float f_num = -k3 * r4 - k3 * r2 - k2 * q * r2 - k1 * q2 * r2 - k1 * q2 + k1 * r4 + k1 * r2 - q2 * q;
      const float f_den = I.fx * q * (k2 * r4 - 2.0f * k1 * q * r2 + q2);
      dX[0] = ub * f_num / f_den;
      dY[0] = vb * f_num / f_den;
      if constexpr (F > 1) {
        const float tt = -k1 * (r2 + 1.0f) + k1 + q;
        const float k_num = (k1 + q) * (k1 * r2 + q * (r2 + 1.0f) - q) - (k1 * r2 - q) * tt;
        const float k_den = q * tt * tt;
        dX[1] = ub * k_num / k_den;
        dY[1] = vb * k_num / k_den;
      }
    }
  }
}

// projection of X1 = (X,Y,Z) with the z < MIN_DEPTH -> 1 clamp (cameras.py:175-177, 297-298).
// Jp = d(x,y)/d(X,Y,Z) (2x3; the 4th column is zero), Jf = d(x,y)/d(intrinsic f) at the TARGET view.
template <int CAM, bool JAC, int F>
__device__ __forceinline__ void proj(const Intr& I, float X, float Y, float Zin, float& x, float& y,
                                     float (&Jp)[2][3], float (&Jf)[2][F > 0 ? F : 1]) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) {
    // an invalid point (weight 0 in the BA, valid 0 from reproject) is replaced by the forward axis: everything stays finite
    const bool ok = valid_point<CAM>(X, Y, Zin);
    const float Xv = ok ? X : 0.0f, Yv = ok ? Y : 0.0f, Zv = ok ? Zin : 1.0f;
    const float rho2 = Xv * Xv + Zv * Zv, r2 = rho2 + Yv * Yv;
    const float rho = sqrtf(rho2);
    x = atan2f(Xv, Zv) * I.fx + (0.5f * I.cx - 0.5f);
    if (x >= I.cx - 0.5f) x -= I.cx;  // theta == pi is the seam: column -0.5
    y = atan2f(rho, -Yv) * I.fy - 0.5f;
    if constexpr (JAC) {
      const float ix = I.fx / rho2, iy = I.fy / (rho * r2);
      Jp[0][0] = ix * Zv; Jp[0][1] = 0.0f; Jp[0][2] = -ix * Xv;
      Jp[1][0] = -iy * Yv * Xv; Jp[1][1] = I.fy * rho / r2; Jp[1][2] = -iy * Yv * Zv;
    }
    if constexpr (F > 0) {
#pragma unroll
      for (int f = 0; f < F; ++f) Jf[0][f] = Jf[1][f] = 0.0f;
    }
    return;
  }
  const float Z = Zin < MIN_DEPTH ? 1.0f : Zin;
  if constexpr (CAM == VIPE_CAM_PINHOLE) {
    const float d = 1.0f / Z;
    x = I.fx * (X * d) + I.cx;
    y = I.fy * (Y * d) + I.cy;
    if constexpr (JAC) {
      Jp[0][0] = I.fx * d; Jp[0][1] = 0.0f; Jp[0][2] = -I.fx * X * d * d;
      Jp[1][0] = 0.0f; Jp[1][1] = I.fy * d; Jp[1][2] = -I.fy * Y * d * d;
    }
    if constexpr (F > 0) {
      Jf[0][0] = X * d;
      Jf[1][0] = Y * d;
    }
  } else {
    const float k1 = I.k1;
    const float r = sqrtf(X * X + Y * Y + Z * Z);
    const float rbase = Z + k1 * r;
    const float d = 1.0f / rbase;
    x = I.fx * (X * d) + I.cx;
    y = I.fy * (Y * d) + I.cy;
    if constexpr (JAC) {
      const float rd = rbase * rbase * r;
      Jp[0][0] = I.fx * (-k1 * X * X + rbase * r) / rd;
      Jp[0][1] = -I.fx * k1 * X * Y / rd;
      Jp[0][2] = -I.fx * X * (k1 * Z + r) / rd;
      Jp[1][0] = -I.fy * k1 * X * Y / rd;
      Jp[1][1] = I.fy * (-k1 * Y * Y + rbase * r) / rd;
      Jp[1][2] = -I.fy * Y * (k1 * Z + r) / rd;
    }
    if constexpr (F > 0) {
      Jf[0][0] = X * d;
      Jf[1][0] = Y * d;
      if constexpr (F > 1) {
        Jf[0][1] = -I.fx * r * X * d * d;
        Jf[1][1] = -I.fy * r * Y * d * d;
      }
    }
  }
}

}  // namespace cam
