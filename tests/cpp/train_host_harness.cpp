// train_host_harness.cpp — host/Train.hpp's pure host functions and
// host/Inputs.hpp's model writer for ctypes (tests/train_harness.py; links the
// host library, makes no GPU call).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "Inputs.hpp"
#include "Train.hpp"

using namespace locomouse;

namespace {
std::vector<TrainPoint> points(const int* p, int n) {
  std::vector<TrainPoint> v;
  for (int k = 0; k < n; ++k) v.push_back(TrainPoint{p[3 * k], p[3 * k + 1], p[3 * k + 2]});
  return v;
}
int put(const std::vector<TrainPoint>& v, int* out, int cap) {
  for (size_t k = 0; k < v.size() && (int)k < cap; ++k) {
    out[3 * k] = v[k].frame;
    out[3 * k + 1] = v[k].x;
    out[3 * k + 2] = v[k].y;
  }
  return (int)v.size();
}
}  // namespace

extern "C" {

// seen: n_seen (frame, x, y) triples already taken; returns the number selected (out holds up to cap)
int thh_select_mined(const int* cands, int n_c, const int* labels, int n_l, int r_neg, const int* seen, int n_seen,
                     int* out, int cap) {
  TrainSeen s;
  for (int k = 0; k < n_seen; ++k) s.insert(std::make_tuple(seen[3 * k], seen[3 * k + 1], seen[3 * k + 2]));
  return put(select_mined(points(cands, n_c), points(labels, n_l), r_neg, s), out, cap);
}

int thh_initial_negatives(int feature, int frame, const int* labels, int n_l, const int* view, int rows, int cols,
                          int r_neg, int neg_per_frame, int* out, int cap) {
  return put(initial_negatives(feature, frame, points(labels, n_l), lm_rect{view[0], view[1], view[2], view[3]}, rows,
                               cols, r_neg, neg_per_frame),
             out, cap);
}

// out: c_pos, c_neg, eps, rounds, neg_per_frame; returns 1 with the parser's message in msg when it throws
int thh_parse_spec(const char* spec, double* out, char* msg, int cap) {
  TrainOptions o;
  try {
    parse_train_spec(spec, o);
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return 1;
  }
  out[0] = o.c_pos;
  out[1] = o.c_neg;
  out[2] = o.eps;
  out[3] = o.rounds;
  out[4] = o.neg_per_frame;
  return 0;
}

// The six detectors in the model file's order (paw_side, paw_bottom, tail_side, tail_bottom, snout_side,
// snout_bottom): their weights one after another in w, sizes and biases per detector.
int thh_write_model(const char* path, const double* w, const int* rows, const int* cols, const double* bias) {
  Model M;
  size_t off = 0;
  for (int k = 0; k < 6; ++k) {
    const size_t n = (size_t)rows[k] * cols[k];
    M.w[k].assign(w + off, w + off + n);
    off += n;
    M.detector(k)->rows = rows[k];
    M.detector(k)->cols = cols[k];
    M.detector(k)->bias = bias[k];
  }
  M.rebind();
  try {
    write_model(path, M.m);
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}

// Reads it back through load_model: sizes, biases, and the weights into w (cap doubles); returns 0, or 1 / 2
int thh_load_model(const char* path, double* w, int cap, int* rows, int* cols, double* bias) {
  Model M;
  try {
    load_model(path, M);
  } catch (const std::exception&) {
    return 1;
  }
  size_t off = 0;
  for (int k = 0; k < 6; ++k) {
    rows[k] = M.detector(k)->rows;
    cols[k] = M.detector(k)->cols;
    bias[k] = M.detector(k)->bias;
    if (off + M.w[k].size() > (size_t)cap) return 2;
    std::memcpy(w + off, M.w[k].data(), sizeof(double) * M.w[k].size());
    off += M.w[k].size();
  }
  return 0;
}

}  // extern "C"
