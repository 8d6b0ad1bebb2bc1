// ssvio_amd/host/map.cpp -- see map.hpp
#include "map.hpp"

#include <stdexcept>

namespace ssx::host {

void MapPoint::RemoveActiveObservation(const FeaturePtr& f)
{
  for (auto it = active_observations.begin(); it != active_observations.end(); ++it)
    if (*it == f) {                                     // one entry per feature (mappoint.cpp:33-46)
      active_observations.erase(it);
      --active_observed_times;
      return;
    }
}

void MapPoint::RemoveObservation(const FeaturePtr& f)
{
  for (auto it = observations.begin(); it != observations.end(); ++it)
    if (*it == f) {
      observations.erase(it);
      f->map_point = kNoMapPoint;                       // mappoint.cpp:56
      --observed_times;
      return;
    }
}

FramePtr Map::NewFrame(ImagePtr left, ImagePtr right, double timestamp)
{
  auto f = std::make_shared<Frame>();
  f->left_image = std::move(left);
  f->right_image = std::move(right);
  f->timestamp = timestamp;
  f->frame_id = next_frame_id_++;
  return f;
}

MapPointPtr Map::NewMapPoint(const double* position)
{
  auto mp = std::make_shared<MapPoint>();
  mp->id = next_map_point_id_++;
  for (int i = 0; i < 3; ++i) mp->position[i] = position[i];
  return mp;
}

// keyframe.cpp:11-50: the keyframe shares the frame's left feature objects, becomes their holder, and every feature
// with a live map point is appended to that point's observations
KeyFramePtr Map::CreateKF(const FramePtr& frame)
{
  auto kf = std::make_shared<KeyFrame>();
  kf->key_frame_id = next_key_frame_id_++;
  kf->frame_id = frame->frame_id;
  kf->timestamp = frame->timestamp;
  kf->features_left = frame->features_left;
  if (keep_keyframe_images) kf->left_image = frame->left_image;
  for (auto& feat : kf->features_left) {
    feat->keyframe = (long)kf->key_frame_id;
    if (MapPointPtr mp = Lock(feat)) mp->AddObservation(feat);
  }
  return kf;
}

MapPointPtr Map::Lock(long id) const
{
  if (id < 0) return nullptr;
  auto it = all_map_points_.find((unsigned long)id);
  return it == all_map_points_.end() ? nullptr : it->second;
}

// map.cpp:18-58
void Map::InsertKeyFrame(const KeyFramePtr& kf)
{
  current_keyframe_ = kf;
  last_removed_keyframe_ = -1;
  if (all_key_frames_.count(kf->key_frame_id)) throw std::logic_error("Map::InsertKeyFrame: keyframe id inserted twice");
  all_key_frames_.insert({kf->key_frame_id, kf});
  active_key_frames_.insert({kf->key_frame_id, kf});
  for (auto& feat : kf->features_left)
    if (MapPointPtr mp = Lock(feat)) {
      mp->AddActiveObservation(feat);
      InsertActiveMapPoint(mp);
    }
  if (active_key_frames_.size() > num_active_key_frames_) {
    RemoveOldActiveKeyframe();
    RemoveOldActiveMapPoints();
  }
}

void Map::InsertMapPoint(const MapPointPtr& mp)
{
  if (!all_map_points_.insert({mp->id, mp}).second) throw std::logic_error("Map::InsertMapPoint: map point id inserted twice");
}

void Map::InsertActiveMapPoint(const MapPointPtr& mp) { active_map_points_[mp->id] = mp; }

// map.cpp:89-146.  The window drops the keyframe closest to the current one when it is closer than 0.2 (|log| of the
// relative pose), otherwise the farthest.  The running minimum is only updated in the `else` of the maximum test and
// the ids start at 0 -- kept as they are, together with the unordered_map iteration order they depend on.
void Map::RemoveOldActiveKeyframe()
{
  if (!current_keyframe_) return;
  double max_dis = 0, min_dis = 9999;
  unsigned long max_id = 0, min_id = 0;
  const SE3 Twc = current_keyframe_->pose.inverse();
  for (auto& kv : active_key_frames_) {
    if (kv.second == current_keyframe_) continue;
    const double dis = (kv.second->pose * Twc).log_norm();
    if (dis > max_dis) {
      max_dis = dis; max_id = kv.first;
    } else if (dis < min_dis) {
      min_dis = dis; min_id = kv.first;
    }
  }
  const double min_dis_th = 0.2;
  KeyFramePtr victim = active_key_frames_.at(min_dis < min_dis_th ? min_id : max_id);
  active_key_frames_.erase(victim->key_frame_id);
  last_removed_keyframe_ = (long)victim->key_frame_id;
  for (auto& feat : victim->features_left)
    if (MapPointPtr mp = Lock(feat)) mp->RemoveActiveObservation(feat);
}

void Map::RemoveOldActiveMapPoints()
{
  for (auto it = active_map_points_.begin(); it != active_map_points_.end();)
    it = it->second->active_observed_times == 0 ? active_map_points_.erase(it) : std::next(it);
}

void Map::RemoveMapPoint(const MapPointPtr& mp)
{
  all_map_points_.erase(mp->id);
  active_map_points_.erase(mp->id);
}

// loopclosing.cpp:427-453, pointer for pointer (tools/mapmodel.py: ActiveMap.loop_correct is the same text in Python):
//   both map points alive   every observation of the current map point is appended to the loop map point with AddObservation --
//                           NOT AddActiveObservation: the loop map point does not enter the active map here -- and re-pointed at it;
//                           the current map point leaves the map (RemoveMapPoint).  Its own lists are left as they are, like the
//                           reference leaves them: nothing refers to it any more.
//   otherwise               the current feature is pointed at the loop map point, which may be null (:451).
// One deliberate deviation: when the current feature's map point IS the loop feature's map point (a track that lasted from the
// loop keyframe to the current one), the reference appends to the very list it iterates (:441-446) and never returns.  Such a pair
// is already fused: it is skipped and counted.
// A second one: the reference lets two features of the current keyframe end up on ONE loop map point (two pairs that name the same
// loop feature, or a loop map point another feature of the keyframe already tracks).  The next keyframe would then observe that map
// point twice, which the backend's resident window cannot hold (one observation per keyframe, map point and camera; Backend refuses
// such a keyframe).  The first feature keeps the map point; a later pair that would give it to a second feature is skipped and counted.
Map::LoopFusion Map::FuseLoopMapPoints(const KeyFramePtr& current, const KeyFramePtr& loop, const std::vector<int32_t>& pairs)
{
  LoopFusion out;
  std::unordered_map<unsigned long, const Feature*> holder;            // map point -> the feature of the current keyframe that names it
  for (auto& feat : current->features_left)
    if (MapPointPtr mp = Lock(feat)) holder.emplace(mp->id, feat.get());
  for (size_t i = 0; i + 1 < pairs.size(); i += 2) {
    const FeaturePtr& cur_feat = current->features_left.at((size_t)pairs[i]);
    const FeaturePtr& loop_feat = loop->features_left.at((size_t)pairs[i + 1]);
    MapPointPtr loop_mp = Lock(loop_feat), current_mp = Lock(cur_feat);
    if (loop_mp) {
      auto h = holder.find(loop_mp->id);
      if (h != holder.end() && h->second != cur_feat.get()) { ++out.duplicate_skipped; continue; }
      if (current_mp != loop_mp) holder[loop_mp->id] = cur_feat.get();
    }
    if (current_mp && loop_mp) {
      if (current_mp == loop_mp) { ++out.same_point_skipped; continue; }
      for (auto& feat : current_mp->observations) {
        loop_mp->AddObservation(feat);
        feat->map_point = (long)loop_mp->id;
      }
      RemoveMapPoint(current_mp);
      out.removed.push_back(current_mp->id);
    } else {
      cur_feat->map_point = loop_mp ? (long)loop_mp->id : kNoMapPoint;
    }
  }
  return out;
}

void Map::RetractOutlierMapPoints(const std::vector<unsigned long>& ids)
{
  for (unsigned long id : ids) {
    outlier_map_points_.remove(id);
    if (MapPointPtr mp = Lock((long)id)) mp->is_outlier = false;
  }
}

void Map::RemoveAllOutlierMapPoints()
{
  for (unsigned long id : outlier_map_points_) {
    all_map_points_.erase(id);
    active_map_points_.erase(id);
  }
  outlier_map_points_.clear();
}

}  // namespace ssx::host
