// Device functions of the rotated / axis-aligned BEV overlap and IoU, shared by iou3d_nms.hip (pairwise IoU, NMS) and det_post.hip
// (fused post-processing): ONE statement of the arithmetic, so an NMS decision or a recall IoU is the same bits whichever kernel makes it.
// Per pair the arithmetic follows the reference's fp32 formulation (iou3d_nms_kernel.cu box_overlap :107-233, iou_bev :235-243,
// iou_normal :311-323; iou3d_nms_utils.py boxes_iou3d_gpu :48-78).
#pragma once
#include "btc_common.h"

namespace {

struct Pt {
  float x, y;
};

__device__ __forceinline__ float cross3(Pt p1, Pt p2, Pt p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }

__device__ __forceinline__ bool in_box2d(const float* box, Pt p) {
  const float margin = 1e-2f;
  const float c = cosf(-box[6]), s = sinf(-box[6]);
  const float rx = (p.x - box[0]) * c + (p.y - box[1]) * (-s);
  const float ry = (p.x - box[0]) * s + (p.y - box[1]) * c;
  return fabsf(rx) < box[3] / 2 + margin && fabsf(ry) < box[4] / 2 + margin;
}

__device__ __forceinline__ bool seg_intersection(Pt p1, Pt p0, Pt q1, Pt q0, Pt* ans) {
  if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) && fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) &&
        fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y)))
    return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > 1e-8f) {
    ans->x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans->y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans->x = (b0 * c1 - b1 * c0) / D;
    ans->y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

__device__ __forceinline__ void corners(const float* box, Pt* c /* 5 */) {
  const float hx = box[3] / 2, hy = box[4] / 2, co = cosf(box[6]), si = sinf(box[6]);
  const float lx[4] = {box[0] - hx, box[0] + hx, box[0] + hx, box[0] - hx};
  const float ly[4] = {box[1] - hy, box[1] - hy, box[1] + hy, box[1] + hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k].x = (lx[k] - box[0]) * co + (ly[k] - box[1]) * (-si) + box[0];
    c[k].y = (lx[k] - box[0]) * si + (ly[k] - box[1]) * co + box[1];
  }
  c[4] = c[0];
}

__device__ float box_overlap(const float* a, const float* b) {
  Pt ca[5], cb[5], pts[16], ctr = {0.f, 0.f};
  corners(a, ca);
  corners(b, cb);
  int cnt = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      if (seg_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], &pts[cnt])) {
        ctr.x += pts[cnt].x;
        ctr.y += pts[cnt].y;
        ++cnt;
      }
  for (int k = 0; k < 4; ++k) {
    if (in_box2d(a, cb[k])) {
      ctr.x += cb[k].x;
      ctr.y += cb[k].y;
      pts[cnt++] = cb[k];
    }
    if (in_box2d(b, ca[k])) {
      ctr.x += ca[k].x;
      ctr.y += ca[k].y;
      pts[cnt++] = ca[k];
    }
  }
  if (cnt < 3) return 0.f;  // fewer than three points span no area (the reference's loops then add nothing either)
  ctr.x /= cnt;
  ctr.y /= cnt;
  float ang[16];
  for (int i = 0; i < cnt; ++i) ang[i] = atan2f(pts[i].y - ctr.y, pts[i].x - ctr.x);
  for (int j = 0; j < cnt - 1; ++j)  // the reference's bubble sort (same swaps: it compares the same atan2 values)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        Pt t = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = t;
        float u = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = u;
      }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    const float ax = pts[k].x - pts[0].x, ay = pts[k].y - pts[0].y, bx = pts[k + 1].x - pts[0].x, by = pts[k + 1].y - pts[0].y;
    area += ax * by - ay * bx;
  }
  return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const float* a, const float* b) {
  const float sa = a[3] * a[4], sb = b[3] * b[4], so = box_overlap(a, b);
  return so / fmaxf(sa + sb - so, 1e-8f);
}

__device__ __forceinline__ float iou_normal(const float* a, const float* b) {
  const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
  const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
  const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f), inter = w * h;
  return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, 1e-8f);
}

}  // namespace
