// libgslam_orbhip.so — a GSLAM *application* plugin (GSLAM_REGISTER_APPLICATION, GSLAM/core/GSLAM.h:26-33) that puts
// the MI355X hot path on GSLAM's own message bus, in the place the external ORBSLAM plugin occupies
// (doc/doxygen/4_1_orbslam.dox:10-29):
//     in   "dataset/frame"     FramePtr  (what `gslam play` publishes, plugins/play/main.cpp:16,132)
//          "dataset/status"    int       (5 = FINISHED, plugins/play/main.cpp:5-7)
//     out  "orbhip/curframe"   FramePtr  (what qviz / metric_time / metric_traj subscribe to)
//          "orbhip/map"        MapPtr    (frames + map points after every windowed bundle adjustment)
//          "orbhip/matches"    Svar {id, keypoints, matches, tracked}
// Per frame (BASELINE configs[0] "C1": extract + match to previous + optimizePnP):
//     gray image -> FeatureDetector::detectAndCompute -> MapFrame::setKeyPoints (Map.h:311-312)
//     -> brute-force match against the previous frame (cross-checked, Hamming <= matchMaxDistance)
//     -> Optimizer::optimizePnP on the matched (map point, CameraAnchor) pairs, start = previous pose (Optimizer.h:202-207)
//     -> new keypoints get map points by intersecting their rays with the ground plane z = 0 (the `synthplane` dataset's
//        scene; a monocular front end needs SOME initialisation and this one is exact for that scene)
//     every `orbhip.ba_every` frames: Optimizer::optimize on the last `orbhip.ba_window` frames (Optimizer.h:229).
// With `orbhip.vocabulary <file.gbow>` (GSLAM's own vocabulary format, core/Vocabulary.h:1843-1932) the application also
// does the place-recognition half of the ORBSLAM plugin's front end on the GPU:
//     descriptors -> Vocabulary::transform (libgslam_vocabulary: gh_bow_transform_host) -> BowVector + FeatureVector, kept in
//        an OrbhipFrame (MapFrame::getBoWVector / getFeatureVector, Map.h:322-325) that is what gets published and mapped,
//     OrbhipLoopDetector (LoopDetector, Map.h:382-395): every frame is inserted, candidates = the frames at least
//        `orbhip.loop_gap` frames old, scored in ONE batched call (scoreVocabularyBatch -> gh_bow_score_host), best first,
//     a candidate above `orbhip.loop_score` is brute-force matched; matches whose two features lie in the same vocabulary
//        node (the FeatureVector test of ORB-SLAM's SearchByBoW) are kept, and with at least `orbhip.loop_matches` of them
//        a FrameConnection (Map.h:246-262) is added to both frames and {id, candidate, score, matches} goes out on "orbhip/loop".
//     Consecutive tracked frames are linked by FrameConnections too (matches + child-to-parent SE3).
// It is a minimal tracking front end, not a SLAM system: no relocalisation, no loop CORRECTION, no map management.
//     gslam play -dataset seq.synthplane -autostart 1 orbhip metric_time -slam orbhip
// `orbhip.log <file>` records every input and output of the three plugin calls so that tests can replay them through
// the CPU checker (record layouts: CallLog).  The frame, connection, loop-detector, point and map classes are in
// orbhip_types.h; this file holds the options (OrbhipConfig), the log, the per-frame stages (Tracker) and the entry point.
#include <GSLAM/core/GSLAM.h>
#include <GSLAM/core/Optimizer.h>

#include <atomic>
#include <deque>
#include <fstream>
#include <map>
#include <mutex>
#include <thread>

#include <GSLAM/core/Vocabulary.h>

#include "FeatureDetector.h"
#include "orbhip_types.h"

using namespace GSLAM;
using namespace orbhip;

namespace {

typedef std::vector<std::pair<int, int> > Matches;                     // (query keypoint, train keypoint)
typedef std::vector<std::pair<Point3d, CameraAnchor> > Pairs3d;        // (map point, observation) for optimizePnP
typedef std::vector<std::pair<int, int64_t> > PairOwners;              // (keypoint, map point id) of each Pairs3d entry

struct OrbhipConfig {
  int n_features, queue, ba_every, ba_window, min_track;
  double inlier;
  bool track, stop_on_finish, start_dataset;
  std::string log_path, voc_path;
  int loop_gap;
  double loop_score;
  int loop_matches, levels_up;
  std::string save_map;
  int max_iterations;
};

// every `orbhip.*` option: Svar::arg registers name, default and help text, so `gslam orbhip -help` lists them in this order
OrbhipConfig read_config(Svar& config) {
  OrbhipConfig c;
  c.n_features = config.arg<int>("orbhip.nFeatures", 1000, "ORB keypoints per frame");
  c.queue = config.arg<int>("orbhip.queue", 0, "subscriber queue (0 = handle in the publisher's thread)");
  c.ba_every = config.arg<int>("orbhip.ba_every", 10, "windowed bundle adjustment every N frames (0 = never)");
  c.ba_window = config.arg<int>("orbhip.ba_window", 10, "frames in the bundle-adjustment window");
  c.min_track = config.arg<int>("orbhip.min_track", 30, "minimum 3D-2D matches for optimizePnP");
  c.inlier = config.arg<double>("orbhip.inlier", 0.006, "inlier radius of the PnP refit, normalised image units");
  c.track = config.arg<bool>("orbhip.track", true, "run optimizePnP / optimize (false: extract + match only)");
  c.stop_on_finish = config.arg<bool>("orbhip.stop_on_finish", false, "publish messenger/stop when the dataset ends");
  c.start_dataset = config.arg<bool>("orbhip.start_dataset", false,
                                     "publish qviz/start (what the GUI's play button does) until the first frame "
                                     "arrives, so that no frame is lost while the plugins load");
  c.log_path = config.arg<std::string>("orbhip.log", "", "binary record of every plugin call (tests)");
  c.voc_path = config.arg<std::string>("orbhip.vocabulary", "", ".gbow vocabulary: BoW vectors per frame, loop candidates");
  c.loop_gap = config.arg<int>("orbhip.loop_gap", 20, "frames between a query and its oldest-allowed loop candidate");
  c.loop_score = config.arg<double>("orbhip.loop_score", 0.05, "minimum BoW score of a loop candidate");
  c.loop_matches = config.arg<int>("orbhip.loop_matches", 40, "node-consistent matches that make a loop connection");
  c.levels_up = config.arg<int>("orbhip.levels_up", 4, "FeatureVector level (levels up from the leaves)");
  // `.gmap` file (the reference's map format, OrbhipMap::save) rewritten after every bundle adjustment.  The reference's
  // own gmap application would do the same for any published map (plugins/gmap/main.cpp:11-13: Map::save on the "map"
  // topic), but in this snapshot loading it next to `play` makes play's "qviz/open" / frame callbacks fire two and three
  // times (reproduced with reference plugins only), so the application saves its map itself.
  c.save_map = config.arg<std::string>("orbhip.save_map", "", "write the map as a .gmap file after every BA");
  c.max_iterations = config.arg<int>("orbhip.max_iterations", 30, "LM iterations per call");
  return c;
}

struct TrackedFrame {
  FramePtr frame;
  SE3 pose;                      // T_wc
  std::vector<KeyPoint> kps;
  std::vector<Point2d> anchors;  // camera.UnProject(kp.pt).xy (z = 1 plane)
  std::vector<int64_t> pid;      // map point id per keypoint, -1 = none
};

// The binary call log (`orbhip.log <file>`): a sequence of records, each an int32 type followed by the fields below, all
// in host byte order and unpadded.  i = int32, u = uint32, f = float, d = double; a pose is 7 d (qx qy qz qw tx ty tz).
//   1 frame         i id, i n, n KeyPoint (28 bytes each), n x 32 descriptor bytes, i m, m x (i query, i train)
//   2 optimizePnP   i id, i n, n x (3 d point, 2 d observation), pose start, pose result, i ok
//   3 optimize      i id, i cameras, i points, i observations, cameras x (pose, i dof), points x 3 d,
//                   observations x (i camera, i point, 2 d xy)   -- the inputs; then, after the call:
//                   i ok, cameras x pose, points x 3 d
//   4 BoW           i id, i n, n x (u word, f weight), i nodes, nodes x (u node, i k, k x u keypoint)
//   5 loop          i id, i n, n x (i candidate, d score) best first   -- then, after verification of the best one:
//                   i connected frame or -1, i m, m x (i query, i train) node-consistent matches
// Per frame the records come in the order 4, 5, 1, 2 (one per optimizePnP call), 3.  Without a path every method is a
// no-op.  The mutex is for `flush`, which the status handler calls from another thread than the frame handler's.
class CallLog {
 public:
  explicit CallLog(const std::string& path) {
    if (!path.empty()) o_.open(path.c_str(), std::ios::binary);
  }
  void frame(FrameID id, const std::vector<KeyPoint>& kps, const GImage& desc, const Matches& matches) {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    const size_t n = kps.size();
    head(1, id);
    put((int32_t)n);
    if (n) o_.write((const char*)kps.data(), (std::streamsize)(n * sizeof(KeyPoint)));
    if (n) o_.write((const char*)desc.data, (std::streamsize)(n * 32));
    put_matches(matches);
  }
  void pnp(FrameID id, const Pairs3d& m3d, const SE3& start, const SE3& pose, bool ok) {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    head(2, id);
    put((int32_t)m3d.size());
    for (auto& p : m3d) {
      const double r[5] = {p.first.x, p.first.y, p.first.z, p.second.x, p.second.y};
      o_.write((const char*)r, sizeof(r));
    }
    put_pose(start);
    put_pose(pose);
    put((int32_t)(ok ? 1 : 0));
  }
  void ba_inputs(FrameID id, const BundleGraph& g) {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    head(3, id);
    put((int32_t)g.keyframes.size());
    put((int32_t)g.mappoints.size());
    put((int32_t)g.mappointObserves.size());
    for (auto& kf : g.keyframes) {
      put_pose(kf.estimation.get_se3());
      put((int32_t)kf.dof);
    }
    put_points(g);
    for (auto& e : g.mappointObserves) {
      put((int32_t)e.frameId);
      put((int32_t)e.pointId);
      const double m[2] = {e.measurement.x, e.measurement.y};
      o_.write((const char*)m, sizeof(m));
    }
  }
  void ba_result(bool ok, const BundleGraph& g) {  // the second half of record 3; a solve is rare enough to flush after
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    put((int32_t)(ok ? 1 : 0));
    for (auto& kf : g.keyframes) put_pose(kf.estimation.get_se3());
    put_points(g);
    o_.flush();
  }
  void bow(FrameID id, const BowVector& bow, const FeatureVector& feat) {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    head(4, id);
    put((int32_t)bow.size());
    for (auto& kv : bow) {
      put((uint32_t)kv.first);
      put((float)kv.second);
    }
    put((int32_t)feat.size());
    for (auto& kv : feat) {
      put((uint32_t)kv.first);
      put((int32_t)kv.second.size());
      for (unsigned int i : kv.second) put((uint32_t)i);
    }
  }
  void loop_candidates(FrameID id, const LoopCandidates& cands) {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    head(5, id);
    put((int32_t)cands.size());
    for (auto& c : cands) {
      put((int32_t)c.frameId);
      put((double)c.score);
    }
  }
  void loop_result(int32_t loop_to, const Matches& matches) {  // the second half of record 5
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    put(loop_to);
    put_matches(matches);
  }
  void flush() {
    if (!o_.is_open()) return;
    std::lock_guard<std::mutex> l(mu_);
    o_.flush();
  }

 private:
  template <typename T>
  void put(const T& v) { o_.write((const char*)&v, sizeof(T)); }
  void head(int32_t type, FrameID id) {
    put(type);
    put((int32_t)id);
  }
  void put_pose(const SE3& T) {
    const SO3 r = T.get_rotation();
    const Point3d t = T.get_translation();
    const double p[7] = {r.x, r.y, r.z, r.w, t.x, t.y, t.z};
    o_.write((const char*)p, sizeof(p));
  }
  void put_matches(const Matches& matches) {
    put((int32_t)matches.size());
    for (auto& m : matches) {
      put((int32_t)m.first);
      put((int32_t)m.second);
    }
  }
  void put_points(const BundleGraph& g) {
    for (auto& mp : g.mappoints) {
      const double p[3] = {mp.first.x, mp.first.y, mp.first.z};
      o_.write((const char*)p, sizeof(p));
    }
  }

  std::mutex mu_;
  std::ofstream o_;
};

// ray of a keypoint through the plane z = 0
bool on_plane(const SE3& Twc, const Point2d& a, Point3d& X) {
  const Point3d d = Twc.get_rotation() * Point3d(a.x, a.y, 1.0), c = Twc.get_translation();
  if (!(fabs(d.z) > 1e-9)) return false;
  const double lam = -c.z / d.z;
  if (!(lam > 0)) return false;
  X = c + d * lam;
  return true;
}

// the FeatureVector test of ORB-SLAM's SearchByBoW: the matches whose two features descend to the same vocabulary node
// `levels_up` above the leaves (`fq` / `ft`: node -> keypoints of the query / train frame, `nq` / `nt` their keypoint counts)
Matches node_consistent(const Matches& raw, const FeatureVector& fq, size_t nq, const FeatureVector& ft, size_t nt) {
  std::vector<uint32_t> node_q(nq, 0u), node_t(nt, 0u);
  for (auto& kv : fq)
    for (unsigned int i : kv.second) node_q[i] = (uint32_t)kv.first + 1u;
  for (auto& kv : ft)
    for (unsigned int i : kv.second) node_t[i] = (uint32_t)kv.first + 1u;
  Matches out;
  for (auto& m : raw)
    if (node_q[m.first] != 0u && node_q[m.first] == node_t[m.second]) out.push_back(m);
  return out;
}

// camera.UnProject of every keypoint; no keypoint has a map point yet
void unproject_keypoints(const Camera& cam, TrackedFrame& cur) {
  const size_t n = cur.kps.size();
  cur.anchors.resize(n);
  cur.pid.assign(n, -1);
  for (size_t i = 0; i < n; ++i) {
    const Point3d a = cam.isValid() ? cam.UnProject(Point2d(cur.kps[i].pt.x, cur.kps[i].pt.y)) : Point3d(0, 0, 1);
    cur.anchors[i] = Point2d(a.x / a.z, a.y / a.z);
  }
}

// the pairs that reproject within `inlier` (normalised image units) of their observation under `pose`
void select_inliers(const Pairs3d& m3d, const PairOwners& who, const SE3& pose, double inlier, Pairs3d& in3d, PairOwners& inwho) {
  const SE3 Tcw = pose.inverse();
  for (size_t k = 0; k < m3d.size(); ++k) {
    const Point3d Xc = Tcw * m3d[k].first;
    if (!(Xc.z > 1e-9)) continue;
    const double dx = Xc.x / Xc.z - m3d[k].second.x, dy = Xc.y / Xc.z - m3d[k].second.y;
    if (dx * dx + dy * dy < inlier * inlier) {
      in3d.push_back(m3d[k]);
      inwho.push_back(who[k]);
    }
  }
}

// The front end's state and one frame's way through it.  `on_frame` runs on the thread that delivers "dataset/frame" (the
// publisher's, or the Messenger's worker with `orbhip.queue` > 0); `on_status` and `frames()` may be called from others.
class Tracker {
 public:
  Tracker(const OrbhipConfig& cfg, const FeatureDetectorPtr& det, const OptimizerPtr& opt,
          const std::shared_ptr<Vocabulary>& voc, const std::shared_ptr<OrbhipLoopDetector>& loops)
      : cfg_(cfg), det_(det), opt_(opt), voc_(voc), loops_(loops),
        pub_loop_(messenger.advertise<Svar>("orbhip/loop", 0)),
        pub_frame_(messenger.advertise<MapFrame>("orbhip/curframe", 0)),
        pub_map_(messenger.advertise<Map>("orbhip/map", 0)),
        pub_match_(messenger.advertise<Svar>("orbhip/matches", 0)),
        map_(new OrbhipMap()), log_(cfg.log_path) {}

  int frames() const { return n_frames_; }

  void on_status(int status) {
    if (cfg_.stop_on_finish && status == 5 && n_frames_ > 0) {  // FINISHED (plugins/play/main.cpp:5-7)
      log_.flush();
      messenger.publish("messenger/stop", true);
    }
  }

  void on_frame(FramePtr fr) {
    if (!fr || !fr->cameraNum()) return;
    std::shared_ptr<OrbhipFrame> of;
    if (voc_) {  // the frame that is published and mapped carries the BoW data: the dataset's frame classes cannot
      of.reset(new OrbhipFrame(fr));
      fr = of;
    }
    TrackedFrame cur;
    cur.frame = fr;
    GImage desc;
    Matches matches;
    if (!extract_and_match(cur, desc, matches)) return;
    if (of && desc.rows > 0) recognise_place(of, desc);
    const Camera cam = fr->getCamera(0);
    unproject_keypoints(cam, cur);
    log_.frame(fr->id(), cur.kps, desc, matches);

    int tracked = 0;
    bool have_pose = false;
    if (opt_ && cam.isValid()) {
      have_pose = estimate_pose(cur, matches, tracked);
      if (have_pose)
        keep_frame(cur, of, desc, matches);
      else
        window_.clear();  // lost: start again from the next frame's dataset pose
    }
    last_desc_ = desc.clone();
    const int count = ++n_frames_;

    // windowed bundle adjustment over the frames in the window (the two oldest fixed: the gauge)
    if (opt_ && have_pose && cfg_.ba_every > 0 && count % cfg_.ba_every == 0 && window_.size() >= 3) bundle_adjust(fr->id());
    pub_match_.publish(Svar({{"id", (int)fr->id()}, {"keypoints", (int)cur.kps.size()}, {"matches", (int)matches.size()}, {"tracked", tracked}}));
    pub_frame_.publish(fr);
  }

 private:
  bool extract_and_match(TrackedFrame& cur, GImage& desc, Matches& matches) {
    GImage img = cur.frame->getImage(0, IMAGE_GRAY);
    if (img.empty()) img = cur.frame->getImage(0);
    if (!det_->detectAndCompute(img, cur.kps, desc)) {
      LOG(ERROR) << "orbhip: extraction failed on frame " << cur.frame->id();
      return false;
    }
    cur.frame->setKeyPoints(cur.kps, desc);
    if (!last_desc_.empty() && desc.rows > 0) det_->match(desc, last_desc_, matches);
    return true;
  }

  // BoW / feature vector of the frame, loop candidates in one batched scoring call over every frame that is old enough,
  // verification of the best one; then the frame joins the candidates of later frames
  void recognise_place(const std::shared_ptr<OrbhipFrame>& of, const GImage& desc) {
    BowVector bow;
    FeatureVector feat;
    voc_->transform(desc, bow, feat, cfg_.levels_up);
    of->setBoW(bow, feat);
    log_.bow(of->id(), bow, feat);
    LoopCandidates cands;
    loops_->obtainCandidates(of, cands);
    log_.loop_candidates(of->id(), cands);
    Matches lm;
    const int32_t loop_to = cands.empty() ? -1 : verify_loop(of, desc, feat, cands[0], lm);
    log_.loop_result(loop_to, lm);
    loops_->insertMapFrame(of);
    bow_frames_[of->id()] = of;
  }

  // brute-force matches to the candidate that pass the node test; with `loop_matches` of them the two frames get a
  // FrameConnection and "orbhip/loop" goes out.  Returns the connected frame's id, or -1.
  int32_t verify_loop(const std::shared_ptr<OrbhipFrame>& of, const GImage& desc, const FeatureVector& feat,
                      const LoopCandidate& best, Matches& lm) {
    std::shared_ptr<OrbhipFrame> old = bow_frames_[best.frameId];
    Matches raw;
    if (!old || !det_->match(desc, old->getDescriptor(), raw)) return -1;
    FeatureVector fo;
    old->getFeatureVector(fo);
    lm = node_consistent(raw, feat, (size_t)desc.rows, fo, (size_t)old->keyPointNum());
    if ((int)lm.size() < cfg_.loop_matches) return -1;
    FrameConnectionPtr c(new OrbhipConnection());
    c->setMatches(lm);
    of->addParent(old->id(), c);
    old->addChildren(of->id(), c);
    pub_loop_.publish(Svar({{"id", (int)of->id()}, {"candidate", (int)old->id()}, {"score", best.score}, {"matches", (int)lm.size()}}));
    return (int32_t)old->id();
  }

  // The pose of `cur` and the map points its keypoints inherit.  False: tracking is lost.  `tracked` = 3D-2D pairs used.
  bool estimate_pose(TrackedFrame& cur, const Matches& matches, int& tracked) {
    if (window_.empty()) {
      cur.pose = cur.frame->getPose();  // the gauge: the dataset's pose of the first frame
      return true;
    }
    const TrackedFrame& prev = window_.back();
    Pairs3d m3d;
    PairOwners who;
    for (auto& m : matches) {
      const int64_t id = prev.pid[m.second];
      if (id < 0) continue;
      m3d.push_back(std::make_pair(points_[id], CameraAnchor(cur.anchors[m.first].x, cur.anchors[m.first].y, 1.0)));
      who.push_back(std::make_pair(m.first, id));
    }
    tracked = (int)m3d.size();
    if (tracked < cfg_.min_track) return false;
    SE3 pose = prev.pose;
    const bool ok = pnp_two_rounds(cur.frame->id(), m3d, who, pose);
    tracked = (int)m3d.size();
    if (!ok) return false;
    cur.pose = pose;
    for (auto& w : who) cur.pid[w.first] = w.second;
    return true;
  }

  bool logged_pnp(FrameID id, const Pairs3d& m3d, SE3& pose) {
    const SE3 start = pose;
    const bool ok = opt_->optimizePnP(m3d, pose, UPDATE_KF_SE3, NULL);
    log_.pnp(id, m3d, start, pose, ok);
    return ok;
  }

  // two rounds, as ORB-SLAM's pose optimisation does: Huber-robust fit on every match, then a refit on the matches
  // within `inlier` of the first fit (cross-checked Hamming matches still hold ~7 % wrong pairs on this texture, and a
  // match kept here hands its map point on to the new frame).  `m3d` / `who` leave as the pairs of the last fit.
  bool pnp_two_rounds(FrameID id, Pairs3d& m3d, PairOwners& who, SE3& pose) {
    if (!logged_pnp(id, m3d, pose)) return false;
    Pairs3d in3d;
    PairOwners inwho;
    select_inliers(m3d, who, pose, cfg_.inlier, in3d, inwho);
    if ((int)in3d.size() < cfg_.min_track) return true;  // keep the first fit
    m3d.swap(in3d);
    who.swap(inwho);
    return logged_pnp(id, m3d, pose);
  }

  // a frame with a pose: new map points, the link to the previous tracked frame, the window and the map
  void keep_frame(TrackedFrame& cur, const std::shared_ptr<OrbhipFrame>& of, const GImage& desc, const Matches& matches) {
    cur.frame->setPose(cur.pose);
    std::vector<std::pair<PointID, size_t> > obs;
    for (size_t i = 0; i < cur.pid.size(); ++i) {
      Point3d X;
      if (cur.pid[i] < 0 && on_plane(cur.pose, cur.anchors[i], X)) {  // a keypoint that is not tracked yet
        cur.pid[i] = next_pid_;
        points_[next_pid_++] = X;
      }
      if (cur.pid[i] >= 0) obs.push_back(std::make_pair((PointID)cur.pid[i], i));
    }
    if (of && !window_.empty()) connect_to_previous(of, cur, matches);
    window_.push_back(cur);
    while ((int)window_.size() > cfg_.ba_window) window_.pop_front();
    map_->insertMapFrame(cur.frame);
    map_->setFeatures(cur.frame->id(), cur.kps, desc, obs);
  }

  // FrameConnection child (this frame) -> parent (the previous tracked frame)
  void connect_to_previous(const std::shared_ptr<OrbhipFrame>& of, const TrackedFrame& cur, const Matches& matches) {
    std::shared_ptr<OrbhipFrame> pf = std::dynamic_pointer_cast<OrbhipFrame>(window_.back().frame);
    if (!pf) return;
    FrameConnectionPtr c(new OrbhipConnection());
    Matches m = matches;
    c->setMatches(m);
    SE3 c2p = window_.back().pose.inverse() * cur.pose;
    c->setChild2Parent(c2p);
    of->addParent(pf->id(), c);
    pf->addChildren(of->id(), c);
  }

  // the window as a BundleGraph: every point seen from two frames or more; `slot` = map point id -> index in g.mappoints
  void build_graph(BundleGraph& g, std::map<int64_t, size_t>& slot) {
    g.cameraDOF = UPDATE_CAMERA_NONE;
    std::map<int64_t, int> count;
    for (auto& f : window_)
      for (int64_t id : f.pid)
        if (id >= 0) ++count[id];
    for (auto& kv : count)
      if (kv.second >= 2) {
        slot[kv.first] = g.mappoints.size();
        g.mappoints.push_back(std::make_pair(points_[kv.first], true));
      }
    for (size_t fi = 0; fi < window_.size(); ++fi) {
      KeyFrameEstimzation kf;
      kf.estimation = SIM3(window_[fi].pose, 1.0);
      kf.dof = fi < 2 ? UPDATE_KF_NONE : UPDATE_KF_SE3;  // two fixed frames: pose AND scale gauge of a monocular window
      g.keyframes.push_back(kf);
      for (size_t i = 0; i < window_[fi].pid.size(); ++i) {
        auto it = slot.find(window_[fi].pid[i]);
        if (it == slot.end()) continue;
        BundleEdge e;
        e.pointId = it->second;
        e.frameId = fi;
        e.measurement = CameraAnchor(window_[fi].anchors[i].x, window_[fi].anchors[i].y, 1.0);
        e.information = NULL;
        g.mappointObserves.push_back(e);
      }
    }
  }

  // Optimizer::optimize on the window; on success poses and points are written back, the points enter the map, and the
  // map is published and saved
  void bundle_adjust(FrameID id) {
    BundleGraph g;
    std::map<int64_t, size_t> slot;
    build_graph(g, slot);
    log_.ba_inputs(id, g);
    const bool ok = opt_->optimize(g);
    log_.ba_result(ok, g);
    if (!ok) return;
    for (size_t fi = 0; fi < window_.size(); ++fi) {
      window_[fi].pose = g.keyframes[fi].estimation.get_se3();
      window_[fi].frame->setPose(window_[fi].pose);
    }
    for (auto& kv : slot) {
      points_[kv.first] = g.mappoints[kv.second].first;
      map_->insertMapPoint(PointPtr(new OrbhipPoint((PointID)kv.first, points_[kv.first])));
    }
    pub_map_.publish(std::static_pointer_cast<Map>(map_));
    if (!cfg_.save_map.empty() && !map_->save(cfg_.save_map)) LOG(ERROR) << "orbhip: cannot write " << cfg_.save_map;
  }

  const OrbhipConfig cfg_;
  FeatureDetectorPtr det_;
  OptimizerPtr opt_;  // null: extract + match only
  std::shared_ptr<Vocabulary> voc_;
  std::shared_ptr<OrbhipLoopDetector> loops_;
  std::map<FrameID, std::shared_ptr<OrbhipFrame> > bow_frames_;  // frames by id (loop candidates are looked up here)
  Publisher pub_loop_, pub_frame_, pub_map_, pub_match_;
  std::shared_ptr<OrbhipMap> map_;
  std::map<int64_t, Point3d> points_;  // map point id -> world position
  std::deque<TrackedFrame> window_;
  GImage last_desc_;
  int64_t next_pid_ = 1;
  std::atomic<int> n_frames_{0};
  CallLog log_;
};

// vocabulary plugin (libgslam_vocabulary.so: the subclass of GSLAM::Vocabulary whose transforms and batched scoring run on the GPU)
bool load_vocabulary(const OrbhipConfig& cfg, std::shared_ptr<Vocabulary>& voc, std::shared_ptr<OrbhipLoopDetector>& loops) {
  typedef std::shared_ptr<Vocabulary> (*factory_t)(const char*);
  SharedLibraryPtr lib = Registry::get(svar.GetString("VocabularyPlugin", "libgslam_vocabulary"));
  factory_t f = lib ? (factory_t)lib->getSymbol("createVocabularyInstance") : NULL;
  OrbhipLoopDetector::score_fn sf = lib ? (OrbhipLoopDetector::score_fn)lib->getSymbol("scoreVocabularyBatch") : NULL;
  if (f) voc = f(cfg.voc_path.c_str());
  if (!voc || !sf) {
    LOG(ERROR) << "orbhip: cannot load vocabulary " << cfg.voc_path << " through the Vocabulary plugin (svar VocabularyPlugin)";
    return false;
  }
  loops.reset(new OrbhipLoopDetector(voc, sf, cfg.loop_gap, cfg.loop_score));
  return true;
}

}  // namespace

int run_orbhip(Svar config) {
  svar = config;  // alias the host's registry, as every GSLAM application does
  const OrbhipConfig cfg = read_config(config);
  if (config.get("help", false)) return config.help();

  FeatureDetectorPtr det = FeatureDetector::create();
  if (!det) {
    LOG(ERROR) << "orbhip: cannot load the FeatureDetector plugin (svar FeatureDetectorPlugin)";
    return -1;
  }
  det->_config.nFeatures = cfg.n_features;
  det->_config.matchCrossCheck = true;
  OptimizerPtr opt;
  if (cfg.track) {
    opt = Optimizer::create();
    if (!opt) LOG(WARNING) << "orbhip: no Optimizer plugin (svar OptimizerPlugin): tracking disabled";
  }
  if (opt) opt->_config.maxIterations = cfg.max_iterations;
  std::shared_ptr<Vocabulary> voc;
  std::shared_ptr<OrbhipLoopDetector> loops;
  if (!cfg.voc_path.empty() && !load_vocabulary(cfg, voc, loops)) return -1;

  Tracker tracker(cfg, det, opt, voc, loops);
  Subscriber sub = messenger.subscribe("dataset/frame", cfg.queue, [&tracker](FramePtr fr) { tracker.on_frame(fr); });
  Subscriber sub_status = messenger.subscribe("dataset/status", 0, [&tracker](int status) { tracker.on_status(status); });

  LOG(INFO) << "orbhip ready.";
  std::atomic<bool> exiting(false);
  std::thread kick;
  if (cfg.start_dataset)
    kick = std::thread([&]() {
      // `play` only reacts to qviz/start once its dataset is open (plugins/play/main.cpp:30-41); repeat until frames flow
      for (int i = 0; i < 600 && !exiting && tracker.frames() == 0; ++i) {
        messenger.publish("qviz/start", true);
        Rate::sleep(0.1);
      }
    });
  const int rc = Messenger::exec();
  exiting = true;
  if (kick.joinable()) kick.join();
  return rc;
}

GSLAM_REGISTER_APPLICATION(orbhip, run_orbhip);
