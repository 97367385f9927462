// Host module of the device-repose tests (tests/_repose_device_cases.py builds it with g++): the device functions of pt_pose.h,
// one "lane" after the other, against mat_inverse / mat_ne_identity / Box::transform / mat_mul of pt_scene.cpp - the definition
// they are held to - as bit patterns.  pt_scene.cpp is included as text so that the Box of its unnamed namespace can be used.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pt_scene.cpp"

#include "pt_pose.h"

using namespace srt;

namespace {

// equal as bit patterns; two NaNs are equal whatever their sign and payload
bool same_float(float a, float b) {
  if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
  return std::memcmp(&a, &b, sizeof a) == 0;
}
bool same_floats(const float* a, const float* b, int n) {
  for (int i = 0; i < n; i++)
    if (!same_float(a[i], b[i])) return false;
  return true;
}

Mat4 translate_scale_reference(const float pos[3], float scale) {
  Mat4 T = mat_identity(), S = mat_identity();
  T.c[3][0] = pos[0]; T.c[3][1] = pos[1]; T.c[3][2] = pos[2];
  S.c[0][0] = S.c[1][1] = S.c[2][2] = scale;
  return mat_mul(T, S);                      // Mat4::translate(pos) * Mat4::scale(Vec3{scale})
}

}  // namespace

extern "C" {

// Every matrix (16 floats each) with every box (6 floats each).  Returns the number of (matrix, box) pairs in which pose_inverse,
// pose_ne_identity, pose_box or pose_object differs from the host functions in any bit.  seen[0..3]: matrices whose inverse holds
// a NaN / an infinity, matrices with has_trans == 0, posed bounds that are -0.
long pose_emu_mismatches(const float* mats, uint32_t nmats, const float* boxes6, uint32_t nboxes, uint32_t seen[4]) {
  long bad = 0;
  seen[0] = seen[1] = seen[2] = seen[3] = 0;
  for (uint32_t k = 0; k < nmats; k++) {
    Mat4 m;
    std::memcpy(&m, mats + 16 * (size_t)k, sizeof m);
    const Mat4 want_inv = mat_inverse(m);
    const bool want_ne = mat_ne_identity(m);
    float inv[16];
    pose_inverse(mats + 16 * (size_t)k, inv);
    const bool ne = pose_ne_identity(mats + 16 * (size_t)k);
    const bool matrix_ok = same_floats(inv, &want_inv.c[0][0], 16) && ne == want_ne;
    bool any_nan = false, any_inf = false;
    for (int e = 0; e < 16; e++) { any_nan |= std::isnan(inv[e]); any_inf |= std::isinf(inv[e]); }
    seen[0] += any_nan; seen[1] += any_inf; seen[2] += !want_ne;
    for (uint32_t b = 0; b < nboxes; b++) {
      const float* local = boxes6 + 6 * (size_t)b;
      // Box::transform itself, whatever has_trans says
      Box t;
      for (int a = 0; a < 3; a++) { t.mn[a] = local[a]; t.mx[a] = local[3 + a]; }
      t.transform(m);
      float got_t[6];
      std::memcpy(got_t, local, sizeof got_t);
      pose_box(mats + 16 * (size_t)k, got_t);
      // and the three together, as the kernel's lane and the Object ctor / Object::bbox form them
      Mat4 itrans;
      uint32_t has = 0;
      float want_box[6];
      posed_values(m, local, &itrans, &has, want_box);
      PoseOut o;
      std::memset(&o, 0xff, sizeof o);
      pose_object(mats + 16 * (size_t)k, local, &o);
      const bool ok = matrix_ok && same_floats(got_t, t.mn, 3) && same_floats(got_t + 3, t.mx, 3) && std::memcmp(o.trans, &m, sizeof m) == 0 &&
                      same_floats(o.itrans, &itrans.c[0][0], 16) && o.has_trans == has && same_floats(o.box, want_box, 6);
      if (!ok) bad++;
      for (int a = 0; a < 6; a++)
        if (o.box[a] == 0.0f && std::signbit(o.box[a])) seen[3]++;
    }
  }
  return bad;
}

// pose_translate_scale against mat_mul(translate, scale) for n positions (3 floats each): the number that differ in any bit.
long pose_ts_mismatches(const float* pos, uint32_t n, float scale) {
  long bad = 0;
  for (uint32_t k = 0; k < n; k++) {
    const Mat4 want = translate_scale_reference(pos + 3 * (size_t)k, scale);
    float got[16];
    pose_translate_scale(pos + 3 * (size_t)k, scale, got);
    if (std::memcmp(got, &want, sizeof got) != 0) bad++;
  }
  return bad;
}

// mat_mul(translate, scale) itself: 16 floats per position (what a restatement elsewhere is compared with)
void pose_ts_reference(const float* pos, uint32_t n, float scale, float* out16) {
  for (uint32_t k = 0; k < n; k++) {
    const Mat4 want = translate_scale_reference(pos + 3 * (size_t)k, scale);
    std::memcpy(out16 + 16 * (size_t)k, &want, sizeof want);
  }
}

}  // extern "C"
