// StereoRectifier.h — the two cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) calls of System::TrackStereo
// (src/System.cc:260-268) on librgbl_frontend.so.  One object per camera, built once from the maps that
// Settings::precomputeRectificationMaps (src/Settings.cc:485-520) keeps computing on the host with the caller's OpenCV:
//
//   rgbl_shim::StereoRectifier rectL(settings_->M1l(), settings_->M2l(), imLeft.size());
//   rectL.remap(imLeft, imLeftRect);                        // drop-in for cv::remap: host image in, host image out
//   extractor->ExtractRectified(rectL, imLeft.data, ...);   // or: raw image in, keypoints out, one upload (ORBextractor.h)
//
// 8-bit images with 1, 3 or 4 channels; parity with OpenCV 4.x is stated against the restatement in tests/remap_ref.*, unpinned.
#ifndef RGBL_STEREO_RECTIFIER_H
#define RGBL_STEREO_RECTIFIER_H

#include <iostream>

#include "../../include/rgbl_frontend.h"
#include "cv_compat.h"

namespace rgbl_shim {

class StereoRectifier {
 public:
  // M1, M2: CV_32FC1 maps of the rectified image's size; srcSize: the raw image's size
  StereoRectifier(const cv::Mat& M1, const cv::Mat& M2, cv::Size srcSize, int device = 0) {
    if (M1.empty() || M2.empty() || M1.type() != CV_32FC1 || M2.type() != CV_32FC1 || M1.rows != M2.rows || M1.cols != M2.cols ||
        M1.step != M2.step || M1.step % sizeof(float)) {
      std::cerr << "[StereoRectifier] the maps must be two CV_32FC1 matrices of one size and step" << std::endl;
      return;
    }
    mDstW = M1.cols; mDstH = M1.rows; mSrcW = srcSize.width; mSrcH = srcSize.height;
    if (rgbl_rectifier_create(device, mSrcW, mSrcH, mDstW, mDstH, M1.ptr<float>(0), M2.ptr<float>(0), (int)(M1.step / sizeof(float)),
                              &mpHandle) != RGBL_OK) {
      std::cerr << "[StereoRectifier] " << rgbl_last_error() << std::endl;   // the reference reports, it never throws
      mpHandle = nullptr;
    }
  }
  ~StereoRectifier() { rgbl_rectifier_destroy(mpHandle); }
  StereoRectifier(const StereoRectifier&) = delete;
  StereoRectifier& operator=(const StereoRectifier&) = delete;

  bool ok() const { return mpHandle != nullptr; }
  rgbl_rectifier* Handle() const { return mpHandle; }
  int srcWidth() const { return mSrcW; }
  int srcHeight() const { return mSrcH; }
  int dstWidth() const { return mDstW; }
  int dstHeight() const { return mDstH; }

  // cv::remap(src, dst, M1, M2, cv::INTER_LINEAR); false (and a message) when the image does not fit the maps
  bool remap(const cv::Mat& src, cv::Mat& dst) const {
#ifdef RGBL_HAVE_OPENCV
    const int channels = src.channels();
    const bool bytes = src.depth() == CV_8U;
#else
    const int channels = 1;
    const bool bytes = src.type() == CV_8UC1;
#endif
    if (!mpHandle || src.empty() || !bytes || src.cols != mSrcW || src.rows != mSrcH) {
      std::cerr << "[StereoRectifier] remap needs an 8-bit image of the size the maps were built for" << std::endl;
      return false;
    }
    dst.create(mDstH, mDstW, src.type());
    if (rgbl_remap(mpHandle, src.data, channels, (int)src.step, dst.data, (int)dst.step) != RGBL_OK) {
      std::cerr << "[StereoRectifier] " << rgbl_last_error() << std::endl;
      return false;
    }
    return true;
  }

 private:
  rgbl_rectifier* mpHandle = nullptr;
  int mSrcW = 0, mSrcH = 0, mDstW = 0, mDstH = 0;
};

}  // namespace rgbl_shim
#endif
