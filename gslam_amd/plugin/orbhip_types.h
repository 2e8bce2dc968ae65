// The GSLAM map classes of the orbhip application (orbhip_app.cpp): frame connection, frame, loop detector, map point and
// map, each the reference's interface (GSLAM/core/Map.h) with storage.
#pragma once
#include <GSLAM/core/GSLAM.h>
#include <GSLAM/core/Vocabulary.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace orbhip {

using namespace GSLAM;

// FrameConnection (Map.h:246-262) with storage: the matches of a frame pair and, when known, the child-to-parent motion.
class OrbhipConnection : public FrameConnection {
 public:
  std::string type() const override { return "OrbhipConnection"; }
  int matchesNum() override { return (int)matches_.size(); }
  bool getMatches(std::vector<std::pair<int, int> >& m) override { m = matches_; return true; }
  bool getChild2Parent(SE3& T) override { if (has_pose_) T = c2p_; return has_pose_; }
  bool getChild2Parent(SIM3& S) override { if (has_pose_) S = SIM3(c2p_, 1.0); return has_pose_; }
  bool setMatches(std::vector<std::pair<int, int> >& m) override { matches_ = m; return true; }
  bool setChild2Parent(SE3& T) override { c2p_ = T; has_pose_ = true; return true; }
  bool setChild2Parent(SIM3& S) override { c2p_ = S.get_se3(); has_pose_ = true; return true; }

 private:
  std::vector<std::pair<int, int> > matches_;
  SE3 c2p_;
  bool has_pose_ = false;
};

// The frame the application publishes and maps when a vocabulary is configured: the dataset's frame (image, camera) plus
// what the front end computed -- keypoints, descriptors, BoW / feature vectors, connections.
class OrbhipFrame : public MapFrame {
 public:
  explicit OrbhipFrame(const FramePtr& src) : MapFrame(src->id(), src->timestamp()), src_(src) { setPose(src->getPoseScale()); }
  std::string type() const override { return "OrbhipFrame"; }
  int cameraNum() const override { return src_->cameraNum(); }
  SE3 getCameraPose(int idx = 0) const override { return src_->getCameraPose(idx); }
  int imageChannels(int idx = 0) const override { return src_->imageChannels(idx); }
  Camera getCamera(int idx = 0) override { return src_->getCamera(idx); }
  GImage getImage(int idx = 0, int mask = IMAGE_UNDEFINED) override { return src_->getImage(idx, mask); }
  int keyPointNum() const override { ReadMutex l(mu_); return (int)kps_.size(); }
  bool setKeyPoints(const std::vector<KeyPoint>& k, const GImage& d) override {
    WriteMutex l(mu_);
    kps_ = k;
    desc_ = d.clone();
    return true;
  }
  bool getKeyPoints(std::vector<KeyPoint>& k) const override { ReadMutex l(mu_); k = kps_; return true; }
  bool getKeyPoint(int idx, KeyPoint& pt) const override {
    ReadMutex l(mu_);
    if (idx < 0 || idx >= (int)kps_.size()) return false;
    pt = kps_[idx];
    return true;
  }
  bool getKeyPoint(int idx, Point2f& pt) const override {
    ReadMutex l(mu_);
    if (idx < 0 || idx >= (int)kps_.size()) return false;
    pt = kps_[idx].pt;
    return true;
  }
  GImage getDescriptor(int idx = -1) const override {
    ReadMutex l(mu_);
    if (idx < 0) return desc_;
    return idx < desc_.rows ? desc_.row(idx) : GImage();
  }
  bool getBoWVector(BowVector& v) const override { ReadMutex l(mu_); v = bow_; return !bow_.empty(); }
  bool getFeatureVector(FeatureVector& v) const override { ReadMutex l(mu_); v = feat_; return !feat_.empty(); }
  void setBoW(const BowVector& b, const FeatureVector& f) { WriteMutex l(mu_); bow_ = b; feat_ = f; }
  FrameConnectionPtr getParent(FrameID id) const override { ReadMutex l(mu_); auto it = parents_.find(id); return it == parents_.end() ? FrameConnectionPtr() : it->second; }
  FrameConnectionPtr getChild(FrameID id) const override { ReadMutex l(mu_); auto it = children_.find(id); return it == children_.end() ? FrameConnectionPtr() : it->second; }
  bool getParents(FrameConnectionMap& p) const override { ReadMutex l(mu_); p = parents_; return true; }
  bool getChildren(FrameConnectionMap& c) const override { ReadMutex l(mu_); c = children_; return true; }
  bool addParent(FrameID id, const FrameConnectionPtr& c) override { WriteMutex l(mu_); parents_[id] = c; return true; }
  bool addChildren(FrameID id, const FrameConnectionPtr& c) override { WriteMutex l(mu_); children_[id] = c; return true; }
  bool eraseParent(FrameID id) override { WriteMutex l(mu_); return parents_.erase(id) > 0; }
  bool eraseChild(FrameID id) override { WriteMutex l(mu_); return children_.erase(id) > 0; }
  bool clearParents() override { WriteMutex l(mu_); parents_.clear(); return true; }
  bool clearChildren() override { WriteMutex l(mu_); children_.clear(); return true; }

 private:
  FramePtr src_;
  mutable MutexRW mu_;
  std::vector<KeyPoint> kps_;
  GImage desc_;
  BowVector bow_;
  FeatureVector feat_;
  FrameConnectionMap parents_, children_;
};

// LoopDetector (Map.h:382-395) on BoW vectors: all candidates older than `gap` frames are scored in one batched GPU call.
class OrbhipLoopDetector : public LoopDetector {
 public:
  typedef bool (*score_fn)(const Vocabulary*, const BowVector*, const BowVector* const*, int, double*);
  OrbhipLoopDetector(const std::shared_ptr<Vocabulary>& voc, score_fn score, int gap, double min_score)
      : voc_(voc), score_(score), gap_(gap), min_score_(min_score) {}
  std::string type() const override { return "OrbhipLoopDetector"; }
  bool insertMapFrame(const FramePtr& f) override {
    BowVector v;
    if (!f || !f->getBoWVector(v)) return false;
    entries_.push_back(std::make_pair(f->id(), v));
    return true;
  }
  bool eraseMapFrame(const FrameID& id) override {
    for (size_t i = 0; i < entries_.size(); ++i)
      if (entries_[i].first == id) {
        entries_.erase(entries_.begin() + (long)i);
        return true;
      }
    return false;
  }
  bool obtainCandidates(const FramePtr& f, LoopCandidates& out) override {
    out.clear();
    BowVector q;
    if (!f || !f->getBoWVector(q) || !score_) return false;
    std::vector<const BowVector*> db;
    std::vector<FrameID> ids;
    for (auto& e : entries_)
      if (e.first + (FrameID)gap_ <= f->id()) {  // old enough not to be a neighbour of the query
        db.push_back(&e.second);
        ids.push_back(e.first);
      }
    if (db.empty()) return true;
    std::vector<double> sc(db.size(), 0.0);
    if (!score_(voc_.get(), &q, db.data(), (int)db.size(), sc.data())) return false;
    for (size_t i = 0; i < db.size(); ++i)
      if (sc[i] >= min_score_) out.push_back(LoopCandidate(ids[i], sc[i]));
    std::stable_sort(out.begin(), out.end(), [](const LoopCandidate& a, const LoopCandidate& b) { return a.score > b.score; });
    return true;
  }

 private:
  std::shared_ptr<Vocabulary> voc_;
  score_fn score_;
  int gap_;
  double min_score_;
  std::vector<std::pair<FrameID, BowVector> > entries_;
};

class OrbhipPoint : public MapPoint {
 public:
  OrbhipPoint(PointID id, const Point3d& p) : MapPoint(id, p) {}
  std::string type() const override { return "OrbhipPoint"; }
};

class OrbhipMap : public Map {
 public:
  std::string type() const override { return "OrbhipMap"; }
  bool insertMapPoint(const PointPtr& p) override { WriteMutex l(mu_); points_[p->id()] = p; return true; }
  bool insertMapFrame(const FramePtr& f) override { WriteMutex l(mu_); frames_[f->id()] = f; return true; }
  std::size_t frameNum() const override { ReadMutex l(mu_); return frames_.size(); }
  std::size_t pointNum() const override { ReadMutex l(mu_); return points_.size(); }
  FramePtr getFrame(const FrameID& id) const override {
    ReadMutex l(mu_);
    auto it = frames_.find(id);
    return it == frames_.end() ? FramePtr() : it->second;
  }
  PointPtr getPoint(const PointID& id) const override {
    ReadMutex l(mu_);
    auto it = points_.find(id);
    return it == points_.end() ? PointPtr() : it->second;
  }
  bool getFrames(FrameArray& frames) const override {
    ReadMutex l(mu_);
    for (auto& kv : frames_) frames.push_back(kv.second);
    return true;
  }
  bool getPoints(PointArray& points) const override {
    ReadMutex l(mu_);
    for (auto& kv : points_) points.push_back(kv.second);
    return true;
  }

  // what the front end knows about a frame beyond the frame object itself: keypoints, descriptors and which map point
  // each keypoint observes (dataset frame classes such as the reference's FrameMono keep none of it)
  void setFeatures(FrameID id, const std::vector<KeyPoint>& kps, const GImage& desc,
                   const std::vector<std::pair<PointID, size_t> >& obs) {
    WriteMutex l(mu_);
    FrameData& d = features_[id];
    d.kps = kps;
    d.desc = desc.clone();
    d.obs = obs;
  }

  // The reference's map file (`.gmap`: "Hash" / "binary", GSLAM/plugins/gmap/MapHash.cpp:278-360 writes it, :363-445 reads
  // it): so that `gslam orbhip gmap play ... -map orbhip/map -out map.gmap` (the reference's own gmap application calls
  // Map::save on whatever map is published, plugins/gmap/main.cpp:11-13) leaves a file GSLAM's MapHash::load, its gmap
  // viewer and its evaluation tools read.  Field order and raw-struct encoding are the reference's OutStream
  // (:207-236: every value as its in-memory bytes, vectors as size_t count + elements, GImage as cols rows flags + data,
  // strings as size_t length + bytes).  Unlike the reference (which writes empty images there) the descriptors are kept.
  bool save(std::string path) const override {
    if (path.empty() || path.find(".gmap") == std::string::npos) return false;
    std::ofstream ofs(path.c_str(), std::ios::out | std::ios::binary);
    if (!ofs.is_open()) return false;
    ReadMutex l(mu_);
    ofs << "Hash" << std::endl << "binary" << std::endl;
    GmapOut out = {ofs};
    out.value(frames_.size());
    out.value(points_.size());
    for (auto& kv : points_) save_point(out, *kv.second);
    static const FrameData none;
    for (auto& kv : frames_) {
      auto fit = features_.find(kv.first);
      save_frame(out, *kv.second, fit == features_.end() ? none : fit->second);
    }
    return ofs.good();
  }

 private:
  struct FrameData {
    std::vector<KeyPoint> kps;
    GImage desc;
    std::vector<std::pair<PointID, size_t> > obs;
  };
  // the encodings of the reference's OutStream that the two records use
  struct GmapOut {
    std::ofstream& ofs;
    void raw(const void* p, size_t n) { ofs.write((const char*)p, (std::streamsize)n); }
    template <typename T>
    void value(const T& v) { raw(&v, sizeof(T)); }
    void image(const GImage& im) {
      const int hdr[3] = {im.cols, im.rows, im.flags};
      raw(hdr, sizeof(hdr));
      if (!im.empty()) raw(im.data, (size_t)im.total() * im.elemSize());
    }
    void doubles(const std::vector<double>& v) {
      value(v.size());
      if (!v.empty()) raw(v.data(), v.size() * sizeof(double));
    }
  };

  static void save_point(GmapOut& out, MapPoint& pt) {
    out.value(pt.id());
    out.value(pt.getPose());
    out.value(pt.getNormal());
    out.value(pt.getColor());
    out.value(pt.refKeyframeID());
    out.image(GImage());
  }

  void save_frame(GmapOut& out, MapFrame& fr, const FrameData& fd) const {
    out.value(fr.id());
    out.value(fr.timestamp());
    out.value(fr.getPoseScale());
    out.image(GImage());       // the image itself stays with the dataset
    out.value((size_t)0);      // its file name: an empty string
    out.value(fr.imageChannels(0));
    out.doubles(fr.getCamera(0).getParameters());
    out.doubles(std::vector<double>());  // no GPS
    out.image(fd.desc);
    const size_t nk = fd.kps.size();
    out.value(nk);
    if (nk) out.raw(fd.kps.data(), nk * sizeof(KeyPoint));
    out.value(nk);  // one colour per keypoint (MapHash::load asserts the sizes agree)
    for (size_t i = 0; i < nk; ++i) out.value(ColorType(255, 255, 255));
    // only observations of points that are in the map (a point enters it with its first bundle adjustment)
    std::vector<std::pair<PointID, size_t> > obs;
    for (size_t i = 0; i < fd.obs.size(); ++i)
      if (points_.count(fd.obs[i].first)) obs.push_back(fd.obs[i]);
    out.value(obs.size());
    for (size_t i = 0; i < obs.size(); ++i) out.value(obs[i]);
    out.value((size_t)0);  // children
    out.value((size_t)0);  // parents
  }

  mutable MutexRW mu_;
  std::map<FrameID, FramePtr> frames_;
  std::map<PointID, PointPtr> points_;
  std::map<FrameID, FrameData> features_;
};

}  // namespace orbhip
