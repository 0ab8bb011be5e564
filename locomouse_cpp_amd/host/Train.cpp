// Train.cpp — see Train.hpp.
#include "Train.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>

namespace locomouse {

const char* const kTrainFeatureNames[TF_COUNT] = {"paw_bottom", "snout_bottom", "tail_bottom",
                                                  "paw_side",   "snout_side",   "tail_side"};

int train_feature_from_name(const std::string& name) {
  for (int f = 0; f < TF_COUNT; ++f)
    if (name == kTrainFeatureNames[f]) return f;
  return -1;
}

namespace {

// index into Model::w / Model::detector (the model file's order) of a feature
int model_slot(int feature) {
  static const int slot[TF_COUNT] = {1, 5, 3, 0, 4, 2};
  return slot[feature];
}

bool side_view(int feature) { return feature >= TF_PAW_SIDE; }

uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int chebyshev(const TrainPoint& a, const TrainPoint& b) { return std::max(std::abs(a.x - b.x), std::abs(a.y - b.y)); }

void check(lm_status s, const char* what) {
  if (s != LM_OK) throw std::runtime_error(std::string("train_detectors: ") + what + ": " + lm_last_error());
}

struct Trainer {
  lm_train_ctx* c = nullptr;
  ~Trainer() { lm_train_destroy(c); }
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

void parse_train_spec(const std::string& spec, TrainOptions& opt) {
  std::vector<std::string> part(1);
  for (char ch : spec) {
    if (ch == ':')
      part.emplace_back();
    else
      part.back().push_back(ch);
  }
  const std::string form = "LM_TRAIN: expected c_pos:c_neg:eps:rounds:neg_per_frame, not " + spec + ".";
  if (part.size() > 5) throw std::invalid_argument(form);
  auto real = [&](const std::string& s, const char* name) {
    size_t used = 0;
    double v = 0;
    try {
      v = std::stod(s, &used);
    } catch (const std::exception&) {
      used = 0;
    }
    if (s.empty() || used != s.size() || !(v > 0) || !std::isfinite(v))
      throw std::invalid_argument(std::string("LM_TRAIN: ") + name + " must be a positive number, not " + s + ".");
    return v;
  };
  auto whole = [&](const std::string& s, const char* name, long lo, long hi) {
    long v = 0;
    bool ok = !s.empty() && s.size() <= 9;
    for (char ch : s) {
      if (ch < '0' || ch > '9') ok = false;
      if (ok) v = v * 10 + (ch - '0');
    }
    if (!ok || v < lo || v > hi)
      throw std::invalid_argument(std::string("LM_TRAIN: ") + name + " must be a whole number in " + std::to_string(lo) +
                                  ".." + std::to_string(hi) + ", not " + s + ".");
    return (int)v;
  };
  if (part.size() > 0) opt.c_pos = real(part[0], "c_pos");
  if (part.size() > 1) opt.c_neg = real(part[1], "c_neg");
  if (part.size() > 2) opt.eps = real(part[2], "eps");
  if (part.size() > 3) opt.rounds = whole(part[3], "rounds", 0, 100);
  if (part.size() > 4) opt.neg_per_frame = whole(part[4], "neg_per_frame", 0, 100000);
}

void parse_train_cv_spec(const std::string& spec, TrainOptions& opt) {
  const std::string form = "LM_TRAIN_CV: expected folds:s1,s2,..., not " + spec + ".";
  const size_t colon = spec.find(':');
  if (colon == std::string::npos || spec.find(':', colon + 1) != std::string::npos) throw std::invalid_argument(form);
  const std::string fs = spec.substr(0, colon);
  long folds = 0;
  bool ok = !fs.empty() && fs.size() <= 9;
  for (char ch : fs) {
    if (ch < '0' || ch > '9') ok = false;
    if (ok) folds = folds * 10 + (ch - '0');
  }
  if (!ok || folds < 2 || folds > 16)
    throw std::invalid_argument("LM_TRAIN_CV: folds must be a whole number in 2..16, not " + fs + ".");
  std::vector<std::string> part(1);
  for (char ch : spec.substr(colon + 1)) {
    if (ch == ',')
      part.emplace_back();
    else
      part.back().push_back(ch);
  }
  std::vector<double> scales;
  for (const std::string& t : part) {
    size_t used = 0;
    double v = 0;
    try {
      v = std::stod(t, &used);
    } catch (const std::exception&) {
      used = 0;
    }
    if (t.empty() || t[0] == ' ' || t[0] == '\t' || used != t.size() || !(v > 0) || !std::isfinite(v))
      throw std::invalid_argument("LM_TRAIN_CV: a scale must be a positive number, not \"" + t + "\".");
    if (std::find(scales.begin(), scales.end(), v) != scales.end())
      throw std::invalid_argument("LM_TRAIN_CV: scale " + t + " is given twice.");
    scales.push_back(v);
  }
  if (scales.size() > 16) throw std::invalid_argument("LM_TRAIN_CV: at most 16 scales, not " + std::to_string(scales.size()) + ".");
  if (folds * (long)scales.size() > LM_TRAIN_MAX_PROBLEMS)
    throw std::invalid_argument("LM_TRAIN_CV: folds x scales must be at most " + std::to_string(LM_TRAIN_MAX_PROBLEMS) +
                                ", not " + std::to_string(folds * (long)scales.size()) + ".");
  opt.cv_folds = (int)folds;
  opt.cv_scales = scales;
}

std::vector<int32_t> cv_fold_of_samples(const std::vector<int>& sample_frames, int folds) {
  std::vector<int> frames = sample_frames;
  std::sort(frames.begin(), frames.end());
  frames.erase(std::unique(frames.begin(), frames.end()), frames.end());
  std::vector<int32_t> out;
  for (int f : sample_frames)
    out.push_back((int32_t)((std::lower_bound(frames.begin(), frames.end(), f) - frames.begin()) % folds));
  return out;
}

namespace {

// The sum of a row's error terms as num / den (the score is half of it).
void cv_fraction(const CvRow& r, __int128& num, __int128& den) {
  if (r.n_pos > 0 && r.n_neg > 0) {
    num = (__int128)r.miss_pos * r.n_neg + (__int128)r.miss_neg * r.n_pos;
    den = (__int128)r.n_pos * r.n_neg;
  } else if (r.n_pos > 0) {
    num = r.miss_pos;
    den = r.n_pos;
  } else if (r.n_neg > 0) {
    num = r.miss_neg;
    den = r.n_neg;
  } else {
    num = 0;
    den = 1;
  }
}

}  // namespace

int cv_select(std::vector<CvRow>& rows) {
  int best = -1;
  __int128 bn = 0, bd = 1;
  for (size_t k = 0; k < rows.size(); ++k) {
    __int128 n, d;
    cv_fraction(rows[k], n, d);
    rows[k].score = 0.5 * ((double)n / (double)d);
    // n / d < bn / bd  <=>  n bd < bn d (counts are below 2^31: the products fit)
    const bool less = best < 0 || n * bd < bn * d;
    const bool equal = best >= 0 && n * bd == bn * d;
    if (less || (equal && rows[k].scale < rows[(size_t)best].scale)) {
      best = (int)k;
      bn = n;
      bd = d;
    }
  }
  return best;
}

std::vector<TrainPoint> select_mined(const std::vector<TrainPoint>& candidates, const std::vector<TrainPoint>& labels,
                                     int r_neg, TrainSeen& seen) {
  std::multimap<int, const TrainPoint*> by_frame;
  for (const TrainPoint& l : labels) by_frame.emplace(l.frame, &l);
  std::vector<TrainPoint> out;
  for (const TrainPoint& c : candidates) {
    const auto key = std::make_tuple(c.frame, c.x, c.y);
    if (seen.count(key)) continue;
    bool near = false;
    const auto range = by_frame.equal_range(c.frame);
    for (auto it = range.first; it != range.second && !near; ++it) near = chebyshev(c, *it->second) < r_neg;
    if (near) continue;
    seen.insert(key);
    out.push_back(c);
  }
  return out;
}

std::vector<TrainPoint> initial_negatives(int feature, int frame, const std::vector<TrainPoint>& labels, lm_rect view,
                                          int rows, int cols, int r_neg, int neg_per_frame) {
  const int x0 = std::max(view.x, 0), y0 = std::max(view.y, 0);
  const int x1 = std::min(view.x + view.width, cols), y1 = std::min(view.y + view.height, rows);
  std::vector<TrainPoint> out;
  if (x1 <= x0 || y1 <= y0) return out;
  const uint64_t key = ((uint64_t)(uint32_t)feature << 56) ^ ((uint64_t)(uint32_t)frame << 24);
  const int64_t tries = 64 * (int64_t)neg_per_frame;
  for (int64_t k = 0; k < tries && (int)out.size() < neg_per_frame; ++k) {
    const uint64_t h = splitmix64(key ^ (uint64_t)k);
    const TrainPoint p{frame, x0 + (int)(h % (uint64_t)(x1 - x0)), y0 + (int)(splitmix64(h) % (uint64_t)(y1 - y0))};
    bool near = false;
    for (const TrainPoint& l : labels)
      if (l.frame == frame && chebyshev(p, l) < r_neg) near = true;
    if (!near) out.push_back(p);
  }
  return out;
}

void check_train_labels(const LocoMouse_Inputs& in, const TrainLabels& labels) {
  const int rows = in.setup.calib_rows, cols = in.setup.calib_cols;
  bool any = false;
  for (int f = 0; f < TF_COUNT; ++f) {
    if (!labels.requested[f]) continue;
    any = true;
    const std::string name = kTrainFeatureNames[f];
    if (labels.points[f].empty()) throw std::invalid_argument("labels_" + name + " is empty or undefined.");
    for (size_t k = 0; k < labels.points[f].size(); ++k) {
      const TrainPoint& p = labels.points[f][k];
      const std::string at = "labels_" + name + " row " + std::to_string(k) + ": ";
      if (p.frame < 0 || (uint32_t)p.frame >= in.n_frames)
        throw std::invalid_argument(at + "frame " + std::to_string(p.frame) + " is outside the video's " +
                                    std::to_string(in.n_frames) + " frames.");
      if (p.x < 0 || p.x >= cols || p.y < 0 || p.y >= rows)
        throw std::invalid_argument(at + "(" + std::to_string(p.x) + ", " + std::to_string(p.y) +
                                    ") is outside the corrected image [" + std::to_string(cols) + " x " +
                                    std::to_string(rows) + "].");
    }
  }
  if (!any) throw std::invalid_argument("no feature to train.");
}

void check_train_cv(const TrainLabels& labels, const TrainOptions& opt) {
  if (opt.cv_folds == 0) return;
  const size_t ns = opt.cv_scales.size();
  if (opt.cv_folds < 2 || opt.cv_folds > 16 || ns < 1 || ns > 16 || (size_t)opt.cv_folds * ns > LM_TRAIN_MAX_PROBLEMS)
    throw std::invalid_argument("LM_TRAIN_CV: folds must be in 2..16, with 1..16 scales and folds x scales at most " +
                                std::to_string(LM_TRAIN_MAX_PROBLEMS) + ".");
  for (size_t k = 0; k < ns; ++k) {
    const double v = opt.cv_scales[k];
    if (!(v > 0) || !std::isfinite(v) || std::count(opt.cv_scales.begin(), opt.cv_scales.end(), v) != 1)
      throw std::invalid_argument("LM_TRAIN_CV: the scales must be positive and finite, each at most once.");
  }
  for (int f = 0; f < TF_COUNT; ++f) {
    if (!labels.requested[f]) continue;
    std::set<int> frames;
    for (const TrainPoint& p : labels.points[f]) frames.insert(p.frame);
    if ((int)frames.size() < opt.cv_folds)
      throw std::invalid_argument(std::string("LM_TRAIN_CV: labels_") + kTrainFeatureNames[f] + " has " +
                                  std::to_string(frames.size()) + " labelled frames, fewer than the " +
                                  std::to_string(opt.cv_folds) + " folds.");
  }
}

namespace {

struct Session {
  const LocoMouse_Inputs& in;
  const TrainOptions& opt;
  std::vector<int> frames;           // the labelled video frames, ascending
  std::map<int, int> index_of;       // video frame -> index into `frames`
  std::vector<uint8_t> pixels;       // those frames, video_rows x video_cols each
  size_t fb = 0;
  TrainReport rep;

  Session(const LocoMouse_Inputs& i, const TrainOptions& o) : in(i), opt(o) {}

  void read_frames() {
    fb = (size_t)in.setup.video_rows * in.setup.video_cols;
    pixels.resize(fb * frames.size());
    if (!in.read_frames && !in.read_frame) throw std::runtime_error("train_detectors: no frame reader");
    const int last = frames.back(), batch = std::max(in.batch, 1);
    std::vector<uint8_t> buf(fb * (size_t)batch);
    size_t next = 0;
    for (int first = 0; first <= last;) {
      const int want = std::min(batch, last + 1 - first);
      int got = 0;
      if (in.read_frames) {
        got = in.read_frames(buf.data(), want);
      } else {
        while (got < want && in.read_frame(buf.data() + (size_t)got * fb)) ++got;
      }
      if (got != want)
        throw std::runtime_error("train_detectors: failed to read frame " + std::to_string(first + std::max(got, 0)) +
                                 " of " + std::to_string(in.n_frames));
      while (next < frames.size() && frames[next] < first + got) {
        std::memcpy(pixels.data() + next * fb, buf.data() + (size_t)(frames[next] - first) * fb, fb);
        ++next;
      }
      first += got;
    }
    if (in.rewind) in.rewind();
  }

  // The LocoMouse mirror over the labelled frames alone, with `model`.
  std::unique_ptr<LocoMouse> mirror(const lm_model& model) {
    LocoMouse_Inputs li = in;
    li.model = model;
    li.n_frames = (uint32_t)frames.size();
    li.devices.clear();
    li.decode = LocoMouse_Inputs::Decode::host;
    li.read_compressed = nullptr;
    li.batch = std::max(1, std::min<int>(in.batch, (int)frames.size()));
    li.output_file.clear();
    li.debug_file.clear();
    li.debug_text.clear();
    li.verbose_debug = false;
    li.preview.path.clear();
    auto pos = std::make_shared<size_t>(0);
    const uint8_t* src = pixels.data();
    const size_t n = frames.size(), bytes = fb;
    li.read_frame = [pos, src, n, bytes](uint8_t* dst) {
      if (*pos >= n) return false;
      std::memcpy(dst, src + *pos * bytes, bytes);
      ++*pos;
      return true;
    };
    li.read_frames = [pos, src, n, bytes](uint8_t* dst, int want) {
      const size_t k = std::min<size_t>((size_t)std::max(want, 0), n - *pos);
      std::memcpy(dst, src + *pos * bytes, k * bytes);
      *pos += k;
      return (int)k;
    };
    li.rewind = [pos] { *pos = 0; };
    std::unique_ptr<LocoMouse> L = LocoMouse_Initialize(li);
    L->getBoundingBox();
    L->initializeFeatureLoop();
    return L;
  }

  // One patch per point through det's read of the frames, in chunks of `batch` frames.
  // `sample_frame` grows by the points' frames in the order their samples are stored.
  void gather(lm_train_ctx* tr, lm_ctx* det, std::vector<TrainPoint> pts, int label, std::vector<int>& sample_frame) {
    const auto t0 = std::chrono::steady_clock::now();
    std::stable_sort(pts.begin(), pts.end(), [](const TrainPoint& a, const TrainPoint& b) { return a.frame < b.frame; });
    for (const TrainPoint& p : pts) sample_frame.push_back(p.frame);
    const int batch = std::max(in.batch, 1);
    std::vector<lm_train_point> chunk;
    for (size_t k = 0; k < pts.size();) {
      const int i0 = index_of.at(pts[k].frame);
      chunk.clear();
      int i1 = i0;
      for (; k < pts.size(); ++k) {
        const int i = index_of.at(pts[k].frame);
        if (i >= i0 + batch) break;
        chunk.push_back(lm_train_point{i - i0, pts[k].x, pts[k].y, label});
        i1 = i;
      }
      check(lm_train_gather(tr, det, pixels.data() + (size_t)i0 * fb, (int64_t)fb, i1 - i0 + 1, chunk.data(),
                            (int32_t)chunk.size()),
            "lm_train_gather");
    }
    rep.gather_s += seconds_since(t0);
  }

  // The feature's candidates of every labelled frame under `model`, in image coordinates.
  std::vector<TrainPoint> detect(const lm_model& model, int feature, std::unique_ptr<LocoMouse>& L) {
    L = mirror(model);
    for (unsigned i = 0; i < L->N_frames(); ++i) {
      L->readFrame();
      L->cropBoundingBox();
      L->detectTail();
      L->detectBottomCandidates();
      L->computeUnaryCostsBottom();
      L->computePairwiseCostsBottom();
      L->detectSideCandidates();
      L->matchBottomSideCandidates();
      L->storePreviousImage();
    }
    const std::vector<std::vector<Candidate>>& lists =
        feature == TF_PAW_BOTTOM     ? L->candidates_bottom_paw()
        : feature == TF_SNOUT_BOTTOM ? L->candidates_bottom_snout()
        : feature == TF_PAW_SIDE     ? L->candidates_side_paw()
                                     : L->candidates_side_snout();
    const bool side = side_view(feature);
    const lm_rect box = side ? L->bb_side_mouse() : L->bb_bottom_mouse();
    const std::vector<uint32_t>& ypos = side ? L->bb_y_side_pos() : L->bb_y_bottom_pos();
    const int rows = in.setup.calib_rows, cols = in.setup.calib_cols;
    std::vector<TrainPoint> out;
    for (size_t i = 0; i < lists.size() && i < frames.size(); ++i)
      for (const Candidate& c : lists[i]) {
        // exportPointTracks' mapping: corner - width + 1 + x
        const int x = (int)(L->bb_x_pos()[i] - (uint32_t)box.width + 1u + (uint32_t)c.p.x);
        const int y = (int)(ypos[i] - (uint32_t)box.height + 1u + (uint32_t)c.p.y);
        if (x < 0 || x >= cols || y < 0 || y >= rows) continue;  // the box may hang over the image's edge
        out.push_back(TrainPoint{frames[i], x, y});
      }
    return out;
  }

  void solve(lm_train_ctx* tr, Model& model, int feature, TrainReport::Feature& fr, double scale = 1.0) {
    const auto t0 = std::chrono::steady_clock::now();
    const int slot = model_slot(feature);
    lm_detector* d = model.detector(slot);
    std::vector<double> W((size_t)d->rows * d->cols);
    double rho = 0;
    // (scale 1 leaves the spec's own costs to the bit)
    check(lm_train_solve(tr, opt.c_pos * scale, opt.c_neg * scale, opt.eps, opt.max_iter, W.data(), &rho, &fr.stats),
          "lm_train_solve");
    model.w[slot] = W;
    model.rebind();
    d->bias = rho;
    rep.solve_s += seconds_since(t0);
  }

  // Scores every scale of opt.cv_scales by cross-validation over the stored
  // samples' frames (Train.hpp) and returns the chosen one.
  double cross_validate(lm_train_ctx* tr, const std::vector<int>& sample_frame, int kh, int kw, TrainReport::Feature& fr) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<int32_t> fold = cv_fold_of_samples(sample_frame, opt.cv_folds);
    check(lm_train_set_groups(tr, fold.data(), (int32_t)fold.size()), "lm_train_set_groups");
    const size_t ns = opt.cv_scales.size();
    std::vector<lm_train_problem> problems;
    for (int f = 0; f < opt.cv_folds; ++f)
      for (double s : opt.cv_scales) problems.push_back(lm_train_problem{opt.c_pos * s, opt.c_neg * s, f, 0});
    std::vector<double> W(problems.size() * (size_t)kh * (size_t)kw), rho(problems.size());
    std::vector<lm_train_heldout> held(problems.size());
    check(lm_train_solve_many(tr, problems.data(), (int32_t)problems.size(), opt.eps, opt.max_iter, W.data(), rho.data(),
                              nullptr, held.data()),
          "lm_train_solve_many");
    fr.cv.assign(ns, CvRow());
    for (size_t q = 0; q < problems.size(); ++q) {
      CvRow& r = fr.cv[q % ns];
      r.scale = opt.cv_scales[q % ns];
      r.n_pos += held[q].n_pos;
      r.n_neg += held[q].n_neg;
      r.miss_pos += held[q].miss_pos;
      r.miss_neg += held[q].miss_neg;
    }
    fr.cv_scale = fr.cv[(size_t)cv_select(fr.cv)].scale;
    rep.cv_s += seconds_since(t0);
    return fr.cv_scale;
  }

  void train_feature(int feature, const std::vector<TrainPoint>& labels, Model& model) {
    TrainReport::Feature fr;
    fr.feature = feature;
    const lm_detector* d = model.detector(model_slot(feature));
    const int kh = d->rows, kw = d->cols;
    const int r_neg = opt.r_neg > 0 ? opt.r_neg : std::max(kh, kw) / 4;
    const bool mine = feature != TF_TAIL_BOTTOM && feature != TF_TAIL_SIDE && opt.rounds > 0;
    std::vector<int> lab_frames;
    for (const TrainPoint& p : labels) lab_frames.push_back(p.frame);
    std::sort(lab_frames.begin(), lab_frames.end());
    lab_frames.erase(std::unique(lab_frames.begin(), lab_frames.end()), lab_frames.end());
    TrainSeen seen;
    std::vector<TrainPoint> negatives;
    const lm_rect view = side_view(feature) ? in.setup.view_box_side : in.setup.view_box_bottom;
    for (int f : lab_frames)
      for (const TrainPoint& p : initial_negatives(feature, f, labels, view, in.setup.calib_rows, in.setup.calib_cols,
                                                   r_neg, opt.neg_per_frame))
        if (seen.insert(std::make_tuple(p.frame, p.x, p.y)).second) negatives.push_back(p);
    fr.n_pos = (int)labels.size();
    fr.n_neg_initial = (int)negatives.size();
    const int64_t room = (int64_t)labels.size() + (int64_t)negatives.size() +
                         (mine ? (int64_t)opt.rounds * 512 * (int64_t)frames.size() : 0);
    Trainer T;
    check(lm_train_create(in.device, kh, kw, (int32_t)std::min<int64_t>(std::max<int64_t>(room, 1), LM_TRAIN_MAX_SAMPLES),
                          &T.c),
          "lm_train_create");
    std::unique_ptr<LocoMouse> L = mirror(model.m);
    std::vector<int> sample_frame;
    gather(T.c, L->context(), labels, 1, sample_frame);
    gather(T.c, L->context(), negatives, -1, sample_frame);
    solve(T.c, model, feature, fr);
    for (int round = 0; mine && round < opt.rounds; ++round) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<TrainPoint> cands = detect(model.m, feature, L);
      // a frame labelled for another feature only may show this one unlabelled: its candidates are not negatives
      cands.erase(std::remove_if(cands.begin(), cands.end(),
                                 [&](const TrainPoint& c) {
                                   return !std::binary_search(lab_frames.begin(), lab_frames.end(), c.frame);
                                 }),
                  cands.end());
      std::vector<TrainPoint> mined = select_mined(cands, labels, r_neg, seen);
      rep.mining_s += seconds_since(t0);
      int32_t n_pos = 0, n_neg = 0;
      check(lm_train_samples(T.c, &n_pos, &n_neg), "lm_train_samples");
      const int64_t left = std::min<int64_t>(room, LM_TRAIN_MAX_SAMPLES) - n_pos - n_neg;
      if ((int64_t)mined.size() > left) mined.resize((size_t)std::max<int64_t>(left, 0));
      fr.mined.push_back((int)mined.size());
      if (mined.empty()) break;
      gather(T.c, L->context(), mined, -1, sample_frame);
      solve(T.c, model, feature, fr);
    }
    if (opt.cv_folds > 0) solve(T.c, model, feature, fr, cross_validate(T.c, sample_frame, kh, kw, fr));
    rep.features.push_back(fr);
  }
};

}  // namespace

void train_detectors(const LocoMouse_Inputs& in, const TrainLabels& labels, const TrainOptions& opt, const Model& base,
                     Model& out, TrainReport* report) {
  check_train_labels(in, labels);
  check_train_cv(labels, opt);
  if (!(opt.c_pos > 0) || !(opt.c_neg > 0) || !(opt.eps > 0) || opt.rounds < 0 || opt.neg_per_frame < 0)
    throw std::invalid_argument("train_detectors: c_pos, c_neg and eps must be positive, rounds and neg_per_frame not negative.");
  Session S(in, opt);
  for (int f = 0; f < TF_COUNT; ++f)
    if (labels.requested[f])
      for (const TrainPoint& p : labels.points[f]) S.frames.push_back(p.frame);
  std::sort(S.frames.begin(), S.frames.end());
  S.frames.erase(std::unique(S.frames.begin(), S.frames.end()), S.frames.end());
  for (size_t i = 0; i < S.frames.size(); ++i) S.index_of[S.frames[i]] = (int)i;
  S.read_frames();
  out = base;
  out.rebind();
  for (int f = 0; f < TF_COUNT; ++f)
    if (labels.requested[f]) S.train_feature(f, labels.points[f], out);
  if (report) *report = S.rep;
}

}  // namespace locomouse
