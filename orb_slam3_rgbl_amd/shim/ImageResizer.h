// ImageResizer.h — the cv::resize(im, imToFeed, settings_->newImSize()) of System::TrackStereo / TrackRGBD / TrackRGBL /
// TrackMonocular (src/System.cc:269-271, 349-351, 486-489, 557-560) on librgbl_frontend.so.  One object per camera size,
// built once from Settings::originalImSize / newImSize:
//
//   rgbl_shim::ImageResizer resizer(settings_->originalImSize(), settings_->newImSize());
//   resizer.resize(im, imToFeed);                              // drop-in for cv::resize: host image in, host image out
//   extractor->ExtractResized(resizer, im.data, ...);          // or: raw image in, keypoints out, one upload (ORBextractor.h)
//
// 8-bit images with 1, 3 or 4 channels, the default INTER_LINEAR; parity with OpenCV 4.x is stated against the restatement in
// tests/resize_ref.py (= the oracle's cv::resize at one channel), unpinned.  The depth map of TrackRGBD (CV_32F / CV_16U) keeps
// its cv::resize.
#ifndef RGBL_IMAGE_RESIZER_H
#define RGBL_IMAGE_RESIZER_H

#include <iostream>

#include "../../include/rgbl_frontend.h"
#include "cv_compat.h"

namespace rgbl_shim {

class ImageResizer {
 public:
  ImageResizer(cv::Size original, cv::Size newSize, int device = 0)
      : mSrcW(original.width), mSrcH(original.height), mDstW(newSize.width), mDstH(newSize.height) {
    if (rgbl_resizer_create(device, mSrcW, mSrcH, mDstW, mDstH, &mpHandle) != RGBL_OK) {
      std::cerr << "[ImageResizer] " << rgbl_last_error() << std::endl;   // the reference reports, it never throws
      mpHandle = nullptr;
    }
  }
  ~ImageResizer() { rgbl_resizer_destroy(mpHandle); }
  ImageResizer(const ImageResizer&) = delete;
  ImageResizer& operator=(const ImageResizer&) = delete;

  bool ok() const { return mpHandle != nullptr; }
  rgbl_resizer* Handle() const { return mpHandle; }
  int srcWidth() const { return mSrcW; }
  int srcHeight() const { return mSrcH; }
  int dstWidth() const { return mDstW; }
  int dstHeight() const { return mDstH; }

  // cv::resize(src, dst, newSize); false (and a message) when the image is not of the original size
  bool resize(const cv::Mat& src, cv::Mat& dst) const {
#ifdef RGBL_HAVE_OPENCV
    const int channels = src.channels();
    const bool bytes = src.depth() == CV_8U;
#else
    const int channels = 1;
    const bool bytes = src.type() == CV_8UC1;
#endif
    if (!mpHandle || src.empty() || !bytes || src.cols != mSrcW || src.rows != mSrcH) {
      std::cerr << "[ImageResizer] resize needs an 8-bit image of the size the resizer was built for" << std::endl;
      return false;
    }
    dst.create(mDstH, mDstW, src.type());
    if (rgbl_resize(mpHandle, src.data, channels, (int)src.step, dst.data, (int)dst.step) != RGBL_OK) {
      std::cerr << "[ImageResizer] " << rgbl_last_error() << std::endl;
      return false;
    }
    return true;
  }

  // Settings::readImageInfo's calibration update (src/Settings.cc:364-404) in its float arithmetic: rows scale fy and cy,
  // columns scale fx and cx (the reference applies it only where it does not rectify).
  void ScaleCalibration(float& fx, float& fy, float& cx, float& cy) const {
    const float scaleRowFactor = (float)mDstH / (float)mSrcH, scaleColFactor = (float)mDstW / (float)mSrcW;
    fy = fy * scaleRowFactor; cy = cy * scaleRowFactor;
    fx = fx * scaleColFactor; cx = cx * scaleColFactor;
  }
  // ... and of a KannalaBrandt8 stereo rig's mvLappingArea (Settings.cc:396-402): columns.  The reference stores the two as int
  // (`int *= float`): assign the float product back to the int to truncate as it does.
  void ScaleLappingArea(float& lap0, float& lap1) const {
    const float scaleColFactor = (float)mDstW / (float)mSrcW;
    lap0 = lap0 * scaleColFactor; lap1 = lap1 * scaleColFactor;
  }

 private:
  rgbl_resizer* mpHandle = nullptr;
  int mSrcW = 0, mSrcH = 0, mDstW = 0, mDstH = 0;
};

}  // namespace rgbl_shim
#endif
