// The planar hand's step-QP geometry (PlanarHandModel::assemble, contact_models.hpp) spread over the lanes of a wave,
// for the uniform-geometry sample pass (smooth_ug.hip, the only unit that includes this file).
//
// assemble is one serial stream -- four sine/cosine pairs, four link-disc pairs with a square root and two divisions
// each, eight rows of J -- that a wave runs with every lane doing the same.  Here lane l acts as r = l & 7 (every
// 8-lane group computes the same, so nothing is masked):
//   angle   r >> 1       a1 (link 0) or a1 + a2 (link 1) of arm r >> 2: one irs_sincos per lane
//   pair    r >> 1       the lane's own sine/cosine is the segment's direction; the arm's first angle comes from lane 0
//                        of the quad (DPP); projection, clamp, closest point, distance, normal, gap, lever arms
//   row     r            generator r & 1 of the pair: e = n +- mu t, the seven entries of J[r], phi[r]
//   k = r                element k of q, D^-1 and b (lane 7: a finite value nobody reads)
// so the dependent chain is one angle -> one pair -> one row instead of four, four and eight.
//
// Every element is the value assemble gives, to the bit: the same operations in the same order, with the compiler's
// contraction of assemble's expressions (-ffp-contract=fast; read from the listing of the unrolled assemble, the same
// for float and double) written out as explicit fma calls.  The unit's flags let the backend fuse any product into a
// sum whatever a pragma says, so every sum or difference here either has no product among its operands or, in the one
// place where assemble rounds the product first (the second joint's height p1y = s1 l1), takes it through
// ug_rounded.  Where the
// unrolled code of link 0 folds a known zero (the segment starts at the arm's base: a = (base, 0), no second lever
// arm), the general form with a zero operand gives the same value, except in two places where the folded form fuses
// differently; both forms are evaluated there and the link's own is selected:
//   ny    link 0: fma(-dy, sp, q1)        link 1: q1 - fma(dy, sp, ay)
//   d^2   link 0: fma(ny, ny, nx nx)      link 1: fma(nx, nx, ny ny)
// (tests/test_smooth_ug_geometry_gpu.py holds the table built on this geometry to the bits of assemble's.)
#pragma once

#include "contact_models.hpp"

__device__ __forceinline__ float ug_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ug_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the value of lane 0 of the lane's quad (quad_perm [0,0,0,0]); all lanes active
__device__ __forceinline__ float ug_quad0(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x00, 0xf, 0xf, true));
}
__device__ __forceinline__ double ug_quad0(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x00, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x00, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// what lane l holds of the geometry, r = l & 7
template <typename T>
struct UgHandLane {
    T J[PlanarHandModel::NX];       // row r of J
    T phi;                          // phi[r]
    T q, Dinv, b;                   // element r of q, D^-1, b (r = 7: unused)
    T kp;                           // the impedance gain behind D^-1[r], r = 3 .. 6
};

// a product that assemble rounds before it is added or subtracted: opaque to the contraction
__device__ __forceinline__ float ug_rounded(float v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ double ug_rounded(double v) { asm volatile("" : "+v"(v)); return v; }

template <typename T>
__device__ __forceinline__ void ug_hand_geometry(const ModelParams& p, const T* x_ext, const T* u, int lane, UgHandLane<T>& o) {
    using M = PlanarHandModel;
    const int r = lane & 7;
    const bool arm1 = (r & 4) != 0, link1 = (r & 2) != 0, gen1 = (r & 1) != 0;
    T q[M::NX];
#pragma unroll
    for (int k = 0; k < M::NX; ++k) q[k] = x_ext[M::perm(k)];
    const T h = T(p.v[0]), g = T(p.v[1]), mass = T(p.v[2]), R = T(p.v[3]), mu = T(p.v[4]);
    const T kp1 = T(p.v[5]), kp2 = T(p.v[6]), l1 = T(p.v[7]), l2 = T(p.v[8]), rl = T(p.v[9]), bx = T(p.v[10]);

    // ---- the lane's angle, its sine and cosine; the arm's first angle's from lane 0 of the quad
    const T a1 = arm1 ? q[5] : q[3] + T(3.14159265358979323846);
    const T a12 = a1 + (arm1 ? q[6] : q[4]);
    T dx, dy;
    irs_sincos(link1 ? a12 : a1, dy, dx);
    const T s1 = ug_quad0(dy), c1 = ug_quad0(dx);

    // ---- the pair: segment start a = (base, 0) + lsel (c1, s1), direction (dx, dy), length L
    const T base = arm1 ? bx : -bx;
    const T lsel = link1 ? l1 : T(0);
    const T L = link1 ? l2 : l1;
    const T ax = ug_fma(c1, lsel, base), ay = ug_rounded(s1 * lsel);
    const T rx = q[0] - ax, ry = ug_fma(-s1, lsel, q[1]);
    T sp = ug_fma(ry, dy, rx * dx);                                 // projection on the segment
    sp = sp < T(0) ? T(0) : (sp > L ? L : sp);
    const T wx = ug_fma(dx, sp, ax), wy = ug_fma(dy, sp, ay);       // closest point on the axis
    T nx = q[0] - wx;
    T ny = link1 ? q[1] - wy : ug_fma(-dy, sp, q[1]);
    const T na = link1 ? nx : ny, nb = link1 ? ny : nx;
    const T dist = irs_sqrt(ug_fma(na, na, nb * nb));
    nx = nx / dist; ny = ny / dist;                                 // link -> object
    const T gap = dist - (R + rl);
    const T cx = ug_fma(nx, rl, wx), cy = ug_fma(ny, rl, wy);       // contact point on the link surface
    const T r1x = cx - base, r1y = cy;                              // about the arm base
    const T r2x = cx - ax, r2y = cy - ay;                           // about the second joint (link 1)

    // ---- the row: generator e = n + sgn t, t = (-ny, nx)
    const T sgn = gen1 ? -mu : mu;
    const T ex = ug_fma(-ny, sgn, nx), ey = ug_fma(nx, sgn, ny);
    const T j1 = ug_fma(r1y, ex, -(ey * r1x));
    const T j2 = link1 ? ug_fma(ex, r2y, -(ey * r2x)) : T(0);
    o.phi = gap;
    o.J[0] = ex;
    o.J[1] = ey;
    o.J[2] = ug_fma(ny, ex, -(nx * ey)) * R;
    o.J[3] = arm1 ? T(0) : j1;
    o.J[4] = arm1 ? T(0) : j2;
    o.J[5] = arm1 ? j1 : T(0);
    o.J[6] = arm1 ? j2 : T(0);

    // ---- element r of q, D^-1 = (h^2/m, h^2/m, h^2/I, 1/kp1, 1/kp2, 1/kp1, 1/kp2), b = (0, m g, 0, kp (q - u))
    const T inertia = T(0.5) * mass * R * R;
    const T kp = (r & 1) ? kp1 : kp2;                               // r = 3, 5: kp1; 4, 6: kp2
    const T qr = r == 0 ? q[0] : r == 1 ? q[1] : r == 2 ? q[2] : r == 3 ? q[3] : r == 4 ? q[4] : r == 5 ? q[5] : q[6];
    const T ur = r == 3 ? u[0] : r == 4 ? u[1] : r == 5 ? u[2] : u[3];
    const T num = r < 3 ? h * h : T(1);
    const T den = r < 2 ? mass : r == 2 ? inertia : kp;
    o.q = qr;
    o.Dinv = num / den;
    o.b = r < 3 ? (r == 1 ? mass * g : T(0)) : kp * (qr - ur);
    o.kp = kp;
}
