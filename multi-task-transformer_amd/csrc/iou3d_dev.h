// Device functions of the bird's-eye-view rotated-box overlap / IoU (the geometric algorithm of csrc/iou3d.hip's header comment), shared by
// the pairwise / NMS kernels of iou3d.hip and the segmented NMS of det_decode.hip so that both suppress exactly the same pairs.
// Include after mtt_device.h, inside the including file's anonymous namespace.  Floating-point contraction is OFF from here to the end of the including file.
#pragma once

#pragma clang fp contract(off)     // same rounding sequence as the (non-fused) restatement the goldens were generated with

constexpr float EPS_ = 1e-8f, MARGIN_ = 1e-5f;
struct P2 { float x, y; };

MTT_DEV float cr3(P2 p1, P2 p2, P2 p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }

MTT_DEV void corners(const float* box, P2 (&c)[5]) {
  const float cx = (box[0] + box[2]) / 2, cy = (box[1] + box[3]) / 2;
  const float cs = cosf(box[4]), sn = sinf(box[4]);
  const float xs[4] = {box[0], box[2], box[2], box[0]}, ys[4] = {box[1], box[1], box[3], box[3]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dx = xs[k] - cx, dy = ys[k] - cy;
    c[k].x = dx * cs + dy * sn + cx;
    c[k].y = -dx * sn + dy * cs + cy;
  }
  c[4] = c[0];
}

MTT_DEV bool in_box(const float* box, P2 p) {
  const float cx = (box[0] + box[2]) / 2, cy = (box[1] + box[3]) / 2;
  const float cs = cosf(-box[4]), sn = sinf(-box[4]);
  const float dx = p.x - cx, dy = p.y - cy;
  const float rx = dx * cs + dy * sn + cx, ry = -dx * sn + dy * cs + cy;
  return rx > box[0] - MARGIN_ && rx < box[2] + MARGIN_ && ry > box[1] - MARGIN_ && ry < box[3] + MARGIN_;
}

MTT_DEV bool seg_x(P2 p1, P2 p0, P2 q1, P2 q0, P2& ans) {
  if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
        fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y))) return false;
  const float s1 = cr3(q0, p1, p0), s2 = cr3(p1, q1, p0), s3 = cr3(p0, q1, q0), s4 = cr3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cr3(q1, p1, p0);
  if (fabsf(s5 - s1) > EPS_) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / D;
    ans.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

MTT_DEV float overlap_area(const float* A, const float* B) {
  P2 ca[5], cb[5], pts[16];
  corners(A, ca);
  corners(B, cb);
  int n = 0;
  float sx = 0.f, sy = 0.f;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 ip;
      if (seg_x(ca[i + 1], ca[i], cb[j + 1], cb[j], ip)) { pts[n++] = ip; sx += ip.x; sy += ip.y; }
    }
  for (int k = 0; k < 4; ++k) {
    if (in_box(A, cb[k])) { pts[n++] = cb[k]; sx += cb[k].x; sy += cb[k].y; }
    if (in_box(B, ca[k])) { pts[n++] = ca[k]; sx += ca[k].x; sy += ca[k].y; }
  }
  if (n == 0) return 0.f;
  const float mx = sx / n, my = sy / n;
  float ang[16];
  for (int k = 0; k < n; ++k) ang[k] = atan2f(pts[k].y - my, pts[k].x - mx);
  for (int j = 0; j < n - 1; ++j)                    // the reference's bubble sort (strict >): the order of equal angles is part of the result
    for (int i = 0; i < n - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        const P2 tp = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = tp;
        const float ta = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = ta;
      }
  float area = 0.f;
  for (int k = 0; k < n - 1; ++k)
    area += (pts[k].x - pts[0].x) * (pts[k + 1].y - pts[0].y) - (pts[k].y - pts[0].y) * (pts[k + 1].x - pts[0].x);
  return fabsf(area) / 2.0f;
}

MTT_DEV float iou_rot(const float* A, const float* B) {
  const float sa = (A[2] - A[0]) * (A[3] - A[1]), sb = (B[2] - B[0]) * (B[3] - B[1]);
  const float ov = overlap_area(A, B);
  return ov / fmaxf(sa + sb - ov, EPS_);
}
MTT_DEV float iou_axis(const float* a, const float* b) {
  const float w = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f), h = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
  const float inter = w * h;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]), sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / fmaxf(sa + sb - inter, EPS_);
}
