"""Host-side mirror of the reference's front-end classes on top of the C ABI.

Same names, argument meaning and error behaviour as the reference C++ classes (the C++ drop-in shims live
in orb_slam3_rgbl_amd/shim/); this Python mirror exists so the parity tests read like calls into
ORB_SLAM3::ORBextractor / DepthModule / ORBmatcher:

  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)   include/ORBextractor.h:49-83
      __call__(image, mask, vLappingArea) -> (keypoints, descriptors, monoIndex)
  DepthModule(params)   .CalculateDepthFromPcd(mvKeys, mvKeysUn, PointCloud, w, h)   include/DepthModule.h:45-99
  ORBmatcher(nnratio, checkOri)  .DescriptorDistance(a, b)  .SearchForTriangulation(...)   include/ORBmatcher.h:40-87

Every compute call goes through the C ABI into the HIP kernels; nothing here computes on the CPU.
`lib=` lets the test-suite hand in a differently bound library (the CPU SIMT emulation of the kernels).
"""
import ctypes as C

import numpy as np

from . import _lib as L

KP_DTYPE = L.KP_DTYPE

UPS_NONE, UPS_NEAREST_NEIGHBOR_PIXEL, UPS_AVERAGE_FILTERING, UPS_INVERSE_DILATION, UPS_IPBASIC = 0, 1, 2, 3, 5
KERNEL_RECT, KERNEL_CROSS, KERNEL_ELLIPSE, KERNEL_DIAMOND = 0, 1, 2, 3


class ORBextractor:
    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, max_batch=1,
                 device=0, lib=None):
        self.lib = lib or L.load()
        cfg = L.ExtractorCfg(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, max_batch)
        self.cfg = cfg
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_extractor_create(C.byref(cfg), device, C.byref(self.h)))
        self.nlevels = nlevels
        self.max_keypoints = self.lib.rgbl_extractor_max_keypoints(self.h)
        n = nlevels
        self.mvScaleFactor, self.mvInvScaleFactor = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.mvLevelSigma2, self.mvInvLevelSigma2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.mnFeaturesPerLevel, self.umax = np.zeros(n, np.int32), np.zeros(16, np.int32)
        L.check(self.lib, self.lib.rgbl_extractor_tables(self.h, L.ptr(self.mvScaleFactor), L.ptr(self.mvInvScaleFactor),
                                                         L.ptr(self.mvLevelSigma2), L.ptr(self.mvInvLevelSigma2),
                                                         L.ptr(self.mnFeaturesPerLevel), L.ptr(self.umax)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_extractor_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # getters of include/ORBextractor.h:61-81
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(self.cfg.scale_factor)

    def GetScaleFactors(self):
        return self.mvScaleFactor

    def GetInverseScaleFactors(self):
        return self.mvInvScaleFactor

    def GetScaleSigmaSquares(self):
        return self.mvLevelSigma2

    def GetInverseScaleSigmaSquares(self):
        return self.mvInvLevelSigma2

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """operator(): returns (keypoints[KP_DTYPE], descriptors[n,32] u8, monoIndex). Empty image -> monoIndex -1."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), -1
        if image.dtype != np.uint8 or image.ndim != 2:
            raise TypeError("image must be CV_8UC1")  # the reference asserts image.type() == CV_8UC1
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        cap = self.max_keypoints
        kps = np.empty(cap, KP_DTYPE)          # fresh arrays per call: the library fills the first n entries, the caller gets views
        desc = np.empty((cap, 32), np.uint8)
        n, mono = C.c_int(0), C.c_int(-1)
        L.check(self.lib, self.lib.rgbl_extract(self.h, L.ptr(image), w, h, image.strides[0], int(vLappingArea[0]),
                                                int(vLappingArea[1]), L.ptr(kps), L.ptr(desc), cap, C.byref(n),
                                                C.byref(mono)))
        self._begun = None
        return kps[:n.value], desc[:n.value], mono.value

    def Begin(self, image, vLappingArea=(0, 0)):
        """Optional latency hook (rgbl_extract_begin): upload + extraction of `image` are queued and not waited for; the next
        operator() call on the SAME array collects the results.  Work issued in between (DepthModule.PrefetchPointcloud) runs
        next to the extraction.  The array must be contiguous in x and unchanged until then."""
        if image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1:
            raise TypeError("image must be CV_8UC1 with contiguous rows")
        h, w = image.shape
        L.check(self.lib, self.lib.rgbl_extract_begin(self.h, L.ptr(image), w, h, image.strides[0], int(vLappingArea[0]), int(vLappingArea[1])))
        # the library recognises the begun frame by its address: holding the array keeps that address from being reused
        self._begun = image

    def CancelBegin(self):
        """Drops a begun frame that will not be collected (rgbl_extract_cancel)."""
        L.check(self.lib, self.lib.rgbl_extract_cancel(self.h))
        self._begun = None

    def extract_color(self, image, mbRGB, vLappingArea=(0, 0)):
        """Tracking::GrabImageRGBL's cvtColor (Tracking.cc:1567-1580) + operator() on an H x W x {3,4} 8-bit image.
        mbRGB (settings `Camera.RGB`) selects COLOR_RGB(A)2GRAY, otherwise COLOR_BGR(A)2GRAY.
        Returns (keypoints, descriptors, monoIndex, mImGray)."""
        image = np.ascontiguousarray(image, np.uint8)
        h, w, ch = image.shape
        cap = self.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        gray = np.zeros((h, w), np.uint8)
        n, mono = C.c_int(0), C.c_int(-1)
        L.check(self.lib, self.lib.rgbl_extract_color(self.h, L.ptr(image), ch, 0 if mbRGB else 1, w, h, image.strides[0],
                                                      int(vLappingArea[0]), int(vLappingArea[1]), L.ptr(kps), L.ptr(desc), cap,
                                                      C.byref(n), C.byref(mono), L.ptr(gray), gray.strides[0]))
        return kps[:n.value].copy(), desc[:n.value].copy(), mono.value, gray

    def extract_rectified(self, rectifier, image, mbRGB=True, vLappingArea=(0, 0)):
        """System::TrackStereo's cv::remap (System.cc:260-268) + cvtColor + operator() on one RAW H x W[ x {3,4}] 8-bit image:
        one upload, everything else on the device.  Returns (keypoints, descriptors, monoIndex, rectified mImGray)."""
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        cap = self.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        gray = np.zeros((self.cfg.height, self.cfg.width), np.uint8)
        n, mono = C.c_int(0), C.c_int(-1)
        L.check(self.lib, self.lib.rgbl_extract_rectified(self.h, rectifier.h, L.ptr(image), ch, 0 if mbRGB else 1, w, h,
                                                          image.strides[0], int(vLappingArea[0]), int(vLappingArea[1]), L.ptr(kps),
                                                          L.ptr(desc), cap, C.byref(n), C.byref(mono), L.ptr(gray), gray.strides[0]))
        return kps[:n.value].copy(), desc[:n.value].copy(), mono.value, gray

    def extract_resized(self, resizer, image, mbRGB=True, vLappingArea=(0, 0)):
        """System::Track*'s cv::resize to Camera.newWidth/newHeight (System.cc:269-271, 349-351, 486-489, 557-560) + cvtColor +
        operator() on one RAW H x W[ x {3,4}] 8-bit image: one upload, the resize at the image's channel count, everything else on
        the device.  Returns (keypoints, descriptors, monoIndex, resized mImGray)."""
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        cap = self.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        gray = np.zeros((self.cfg.height, self.cfg.width), np.uint8)
        n, mono = C.c_int(0), C.c_int(-1)
        L.check(self.lib, self.lib.rgbl_extract_resized(self.h, resizer.h, L.ptr(image), ch, 0 if mbRGB else 1, w, h,
                                                        image.strides[0], int(vLappingArea[0]), int(vLappingArea[1]), L.ptr(kps),
                                                        L.ptr(desc), cap, C.byref(n), C.byref(mono), L.ptr(gray), gray.strides[0]))
        return kps[:n.value].copy(), desc[:n.value].copy(), mono.value, gray

    def extract_batch(self, images, vLappingArea=(0, 0)):
        """images: [B, H, W] u8 contiguous. Returns list of (keypoints, descriptors, monoIndex)."""
        images = np.ascontiguousarray(images, np.uint8)
        b, h, w = images.shape
        cap = self.max_keypoints
        kps = np.zeros((b, cap), KP_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        mono = np.zeros(b, np.int32)
        L.check(self.lib, self.lib.rgbl_extract_batch(self.h, L.ptr(images), b, w, h, images.strides[1], images.strides[0],
                                                      int(vLappingArea[0]), int(vLappingArea[1]), L.ptr(kps), L.ptr(desc),
                                                      cap, L.ptr(n), L.ptr(mono)))
        return [(kps[i, :n[i]].copy(), desc[i, :n[i]].copy(), int(mono[i])) for i in range(b)]

    # mvImagePyramid (include/ORBextractor.h:83)
    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        L.check(self.lib, self.lib.rgbl_extractor_level_size(self.h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def image_pyramid(self, level, frame=0, with_border=False, blurred=False):
        w, h = self.level_size(level)
        b = 19 if (with_border and not blurred) else 0
        out = np.zeros((h + 2 * b, w + 2 * b), np.uint8)
        L.check(self.lib, self.lib.rgbl_extractor_get_level(self.h, frame, level, int(blurred), int(with_border),
                                                            L.ptr(out), out.strides[0]))
        return out

    def level_candidates(self, level, frame=0):
        n = C.c_int(0)
        L.check(self.lib, self.lib.rgbl_extractor_get_candidates(self.h, frame, level, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), KP_DTYPE)
        L.check(self.lib, self.lib.rgbl_extractor_get_candidates(self.h, frame, level, L.ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def UndistortKeyPoints(self, xy, K, mDistCoef):
        """Frame::UndistortKeyPoints (Frame.cc:837-870): mvKeysUn coordinates for mvKeys coordinates xy [n,2]; K = (fx, fy, cx, cy).
        As in the reference, nothing is computed when mDistCoef[0] == 0."""
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(mDistCoef, np.float32).reshape(-1)
        if d[0] == 0.0:
            return a.copy()
        k = np.ascontiguousarray(K, np.float32)
        out = np.zeros_like(a)
        L.check(self.lib, self.lib.rgbl_undistort_points(self.h, L.ptr(a), len(a), L.ptr(k), L.ptr(d), len(d), L.ptr(out)))
        return out

    def profile(self, enable):
        L.check(self.lib, self.lib.rgbl_extractor_profile(self.h, int(enable)))

    def profile_read(self):
        return L.read_profile(self.lib, self.lib.rgbl_extractor_profile_read, self.h)

    def profile_samples(self):
        return L.read_profile_samples(self.lib, self.lib.rgbl_extractor_profile_read, self.lib.rgbl_extractor_profile_samples, self.h)


class Rectifier:
    """The rectification maps of one camera (Settings::precomputeRectificationMaps' M1 / M2, Settings.cc:485-520) on the device:
    cv::remap(src, dst, M1, M2, cv::INTER_LINEAR) of System::TrackStereo (System.cc:260-268) for 8-bit images with 1, 3 or 4
    channels.  The maps (two float32 arrays of the destination's shape) are read once; src_size = (width, height)."""

    def __init__(self, map_x, map_y, src_size, device=0, lib=None):
        self.lib = lib or L.load()
        mx, my = np.asarray(map_x), np.asarray(map_y)
        if mx.dtype != np.float32 or my.dtype != np.float32 or mx.ndim != 2 or mx.shape != my.shape:
            raise TypeError("maps must be two CV_32FC1 arrays of the same shape")
        if mx.strides != my.strides or mx.strides[1] != 4 or mx.strides[0] % 4:
            mx, my = np.ascontiguousarray(mx), np.ascontiguousarray(my)
        self.dst_h, self.dst_w = mx.shape
        self.src_w, self.src_h = int(src_size[0]), int(src_size[1])
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_rectifier_create(device, self.src_w, self.src_h, self.dst_w, self.dst_h, L.ptr(mx), L.ptr(my),
                                                         mx.strides[0] // 4, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_rectifier_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{src_w, src_h, dst_w, dst_h, staged_tiles, direct_tiles, map_bytes} (rgbl_rectifier_info)."""
        v = [C.c_int() for _ in range(6)]
        b = C.c_longlong()
        L.check(self.lib, self.lib.rgbl_rectifier_info(self.h, *[C.byref(x) for x in v], C.byref(b)))
        names = ("src_w", "src_h", "dst_w", "dst_h", "staged_tiles", "direct_tiles")
        return dict({k: x.value for k, x in zip(names, v)}, map_bytes=b.value)

    def remap(self, image):
        """One host image H x W[ x C] (any row stride) -> the rectified host image (imLeftRect)."""
        if image.dtype != np.uint8 or image.ndim not in (2, 3) or image.strides[-1] != 1 or (image.ndim == 3 and image.strides[1] != image.shape[2]):
            image = np.ascontiguousarray(image, np.uint8)
        ch = 1 if image.ndim == 2 else image.shape[2]
        if image.shape[0] != self.src_h or image.shape[1] != self.src_w:
            raise ValueError("image is %dx%d, the maps were built for %dx%d" % (image.shape[1], image.shape[0], self.src_w, self.src_h))
        out = np.zeros((self.dst_h, self.dst_w) if image.ndim == 2 else (self.dst_h, self.dst_w, ch), np.uint8)
        L.check(self.lib, self.lib.rgbl_remap(self.h, L.ptr(image), ch, image.strides[0], L.ptr(out), out.strides[0]))
        return out

    def remap_batch_device(self, extractor, d_src, batch, channels, src_stride, src_frame_stride, d_dst, dst_stride, dst_frame_stride):
        """Device pointers (ints), enqueued on the extractor's stream: a following cvtColor / extraction of that handle sees the result."""
        L.check(self.lib, self.lib.rgbl_remap_batch_device(self.h, extractor.h, d_src, batch, channels, src_stride, src_frame_stride,
                                                           d_dst, dst_stride, dst_frame_stride))


class Resizer:
    """cv::resize(im, imToFeed, settings_->newImSize()) of the System::Track* entries (System.cc:269-271, 349-351, 486-489,
    557-560) on the device: default INTER_LINEAR, 8-bit images with 1, 3 or 4 channels, any ratio.  src_size and dst_size are
    (width, height); the tables of both axes are built once."""

    def __init__(self, src_size, dst_size, device=0, lib=None):
        self.lib = lib or L.load()
        self.src_w, self.src_h = int(src_size[0]), int(src_size[1])
        self.dst_w, self.dst_h = int(dst_size[0]), int(dst_size[1])
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_resizer_create(device, self.src_w, self.src_h, self.dst_w, self.dst_h, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_resizer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{src_w, src_h, dst_w, dst_h, area_fast, table_bytes} (rgbl_resizer_info)."""
        v = [C.c_int() for _ in range(5)]
        b = C.c_longlong()
        L.check(self.lib, self.lib.rgbl_resizer_info(self.h, *[C.byref(x) for x in v], C.byref(b)))
        names = ("src_w", "src_h", "dst_w", "dst_h", "area_fast")
        return dict({k: x.value for k, x in zip(names, v)}, table_bytes=b.value)

    def resize(self, image):
        """One host image H x W[ x C] (any row stride) -> the resized host image (imToFeed)."""
        if image.dtype != np.uint8 or image.ndim not in (2, 3) or image.strides[-1] != 1 or (image.ndim == 3 and image.strides[1] != image.shape[2]):
            image = np.ascontiguousarray(image, np.uint8)
        ch = 1 if image.ndim == 2 else image.shape[2]
        if image.shape[0] != self.src_h or image.shape[1] != self.src_w:
            raise ValueError("image is %dx%d, the resizer was built for %dx%d" % (image.shape[1], image.shape[0], self.src_w, self.src_h))
        out = np.zeros((self.dst_h, self.dst_w) if image.ndim == 2 else (self.dst_h, self.dst_w, ch), np.uint8)
        L.check(self.lib, self.lib.rgbl_resize(self.h, L.ptr(image), ch, image.strides[0], L.ptr(out), out.strides[0]))
        return out

    def resize_batch_device(self, extractor, d_src, batch, channels, src_stride, src_frame_stride, d_dst, dst_stride, dst_frame_stride):
        """Device pointers (ints), enqueued on the extractor's stream: a following cvtColor / extraction of that handle sees the result."""
        L.check(self.lib, self.lib.rgbl_resize_batch_device(self.h, extractor.h, d_src, batch, channels, src_stride, src_frame_stride,
                                                            d_dst, dst_stride, dst_frame_stride))


def ComputeStereoMatches(extractorLeft, extractorRight, mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight, mb, mbf):
    return prepare_ComputeStereoMatches(extractorLeft, extractorRight, mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight, mb, mbf)()


def prepare_ComputeStereoMatches(extractorLeft, extractorRight, mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight, mb, mbf):
    """Frame::ComputeStereoMatches (src/Frame.cc:901-1071). Both extractors must just have processed the left / right
    image (their device-resident pyramids are read). Returns (mvuRight, mvDepth)."""
    lib = extractorLeft.lib
    kl = np.ascontiguousarray(mvKeys, KP_DTYPE)
    kr = np.ascontiguousarray(mvKeysRight, KP_DTYPE)
    dl = np.ascontiguousarray(mDescriptors, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(mDescriptorsRight, np.uint8).reshape(-1, 32)
    ur = np.full(len(kl), -1, np.float32)
    dp = np.full(len(kl), -1, np.float32)
    args = (extractorLeft.h, extractorRight.h, L.ptr(kl), L.ptr(dl), len(kl), L.ptr(kr), L.ptr(dr), len(kr), float(mb), float(mbf),
            L.ptr(ur), L.ptr(dp))

    def call():
        L.check(lib, lib.rgbl_stereo_matches(*args))
        return ur, dp
    return call


def structuring_element(shape, kw, kh, lib=None):
    lib = lib or L.load()
    out = np.zeros(kw * kh, np.uint8)
    L.check(lib, lib.rgbl_structuring_element(shape, kw, kh, L.ptr(out)))
    return out.reshape(kh, kw)


def projection_matrix(K3x4, Tr4x4, lib=None):
    lib = lib or L.load()
    K = np.ascontiguousarray(K3x4, np.float32)
    T = np.ascontiguousarray(Tr4x4, np.float32)
    out = np.zeros((3, 4), np.float32)
    lib.rgbl_projection_matrix(L.ptr(K), L.ptr(T), L.ptr(out))
    return out


def _keys_xy(a):
    """[k, 2] float32, contiguous: the coordinates of KP_DTYPE records or of a [k, 2] array."""
    if a.dtype == KP_DTYPE:
        out = np.empty((len(a), 2), np.float32)
        out[:, 0] = a["x"]
        out[:, 1] = a["y"]
        return out
    return np.ascontiguousarray(a, np.float32).reshape(-1, 2)


class DepthModule:
    """Mirror of ORB_SLAM3::DepthModule. The YAML keys of Examples/RGB-L/*.yaml arrive as keyword arguments."""

    def __init__(self, LidarProjectionMatrix, width, height, min_dist=5.0, max_dist=200.0, mbf=100.0,
                 method=UPS_INVERSE_DILATION, kernel_type=KERNEL_DIAMOND, kernel_size_u=5, kernel_size_v=7,
                 avg_kernel_size=5, nn_search_distance=7.0, max_points=250000, max_keypoints=8192, max_batch=1,
                 device=0, lib=None):
        self.lib = lib or L.load()
        cfg = L.DepthCfg()
        proj = np.asarray(LidarProjectionMatrix, np.float32).reshape(12)
        for i in range(12):
            cfg.proj[i] = float(proj[i])
        cfg.min_dist, cfg.max_dist, cfg.mbf, cfg.method = min_dist, max_dist, mbf, method
        if kernel_type == KERNEL_DIAMOND:
            kernel_size_v = kernel_size_u  # "not considered in Diamond mode" (KITTI00-02.yaml:82)
        k = structuring_element(kernel_type, kernel_size_u, kernel_size_v, self.lib)
        cfg.kernel_h, cfg.kernel_w = k.shape
        for i, v in enumerate(k.reshape(-1)):
            cfg.kernel[i] = int(v)
        cfg.avg_kernel_size, cfg.nn_search_radius = avg_kernel_size, nn_search_distance
        cfg.width, cfg.height = width, height
        cfg.max_points, cfg.max_keypoints, cfg.max_batch = max_points, max_keypoints, max_batch
        self.cfg = cfg
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_depth_create(C.byref(cfg), device, C.byref(self.h)))
        self.mvDepth = self.mvuRight = self.RawDepthMap = self.ProcessedDepthMap = None

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_depth_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def PrefetchPointcloud(self, PointCloud, imwidth, imheight):
        """Optional latency hook (rgbl_depth_prefetch): upload, projection and up-sampling of the scan are queued and not
        waited for; CalculateDepthFromPcd(..., want_maps=False) on the SAME array then only gathers the keypoints' depths."""
        cloud = PointCloud
        if cloud.dtype != np.float32 or cloud.ndim != 2 or cloud.shape[0] != 4 or cloud.strides[1] != 4:
            raise TypeError("PointCloud must be a 4 x N float32 array with contiguous rows")
        L.check(self.lib, self.lib.rgbl_depth_prefetch(self.h, L.ptr(cloud), cloud.shape[1], cloud.strides[0] // 4, imwidth, imheight))
        self._prefetched = cloud  # the scan is recognised by its address: keep it from being reused until it is consumed

    def CancelPrefetch(self):
        """Forgets a prefetched scan that will not be followed by CalculateDepthFromPcd (rgbl_depth_prefetch_cancel)."""
        L.check(self.lib, self.lib.rgbl_depth_prefetch_cancel(self.h))
        self._prefetched = None

    def CalculateDepthFromPcd(self, mvKeys, mvKeysUn, PointCloud, imwidth, imheight, want_maps=True):
        """mvKeys / mvKeysUn: KP_DTYPE arrays (or [k,2] float arrays); PointCloud: 4 x N float32."""
        kp = _keys_xy(mvKeys)
        un = np.ascontiguousarray(_keys_xy(mvKeysUn)[:, 0])
        cloud = np.asarray(PointCloud, np.float32)
        if cloud.ndim != 2 or cloud.shape[0] != 4:
            raise ValueError("PointCloud must be 4 x N (rows x, y, z, 1)")
        if cloud.strides[1] != 4:
            cloud = np.ascontiguousarray(cloud)
        n, k = cloud.shape[1], kp.shape[0]
        self.mvDepth, self.mvuRight = np.empty(k, np.float32), np.empty(k, np.float32)   # written for every keypoint
        self.RawDepthMap = np.zeros((imheight, imwidth), np.float32) if want_maps else None
        proc_ok = want_maps and self.cfg.method != UPS_NEAREST_NEIGHBOR_PIXEL
        self.ProcessedDepthMap = np.zeros((imheight, imwidth), np.float32) if proc_ok else None
        L.check(self.lib, self.lib.rgbl_depth_compute(self.h, L.ptr(cloud), n, cloud.strides[0] // 4, imwidth, imheight,
                                                      L.ptr(kp), L.ptr(un), k, L.ptr(self.mvDepth), L.ptr(self.mvuRight),
                                                      L.ptr(self.RawDepthMap), L.ptr(self.ProcessedDepthMap)))
        self._prefetched = None

    def CalculateDepthFromKittiBin(self, mvKeys, mvKeysUn, xyzi, imwidth, imheight, want_maps=True):
        """The scan as read from a KITTI velodyne .bin file: N x 4 float32 (x, y, z, reflectance) - what
        LoadPointcloudBinaryMat (Examples/RGB-L/rgbl_kitti.cc:151-185) turns into the 4 x N matrix, without the repack."""
        kp = _keys_xy(mvKeys)
        un = np.ascontiguousarray(_keys_xy(mvKeysUn)[:, 0])
        pts = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        n, k = pts.shape[0], kp.shape[0]
        self.mvDepth, self.mvuRight = np.empty(k, np.float32), np.empty(k, np.float32)
        self.RawDepthMap = np.zeros((imheight, imwidth), np.float32) if want_maps else None
        proc_ok = want_maps and self.cfg.method != UPS_NEAREST_NEIGHBOR_PIXEL
        self.ProcessedDepthMap = np.zeros((imheight, imwidth), np.float32) if proc_ok else None
        L.check(self.lib, self.lib.rgbl_depth_compute_xyzi(self.h, L.ptr(pts), n, imwidth, imheight, L.ptr(kp), L.ptr(un), k,
                                                           L.ptr(self.mvDepth), L.ptr(self.mvuRight), L.ptr(self.RawDepthMap),
                                                           L.ptr(self.ProcessedDepthMap)))

    def SetSparseUpsampling(self, enable):
        """rgbl_depth_set_sparse: an InverseDilation module writes ProcessedDepthMap only for calls that ask for the maps;
        otherwise the dilation is evaluated at the keypoints' pixels.  mvDepth / mvuRight do not change."""
        L.check(self.lib, self.lib.rgbl_depth_set_sparse(self.h, int(bool(enable))))

    def profile(self, enable):
        L.check(self.lib, self.lib.rgbl_depth_profile(self.h, int(enable)))

    def profile_read(self):
        return L.read_profile(self.lib, self.lib.rgbl_depth_profile_read, self.h)

    def profile_samples(self):
        return L.read_profile_samples(self.lib, self.lib.rgbl_depth_profile_read, self.lib.rgbl_depth_profile_samples, self.h)


class DeviceFrame:
    """A Frame / KeyFrame whose per-feature arrays (mDescriptors, mvKeysUn[].pt / .octave, mvuRight) are resident in HBM
    (rgbl_device_frame): filled once - from host arrays or straight from the extractor / depth handles - and named by the
    `device` / `device2` member of the matcher inputs, which then upload nothing for it."""

    def __init__(self, capacity, device=0, lib=None):
        self.lib = lib or L.load()
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_device_frame_create(device, int(capacity), C.byref(self.h)))

    def upload(self, desc, xy, octave, uright=None):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        o = np.ascontiguousarray(octave, np.int32)
        u = None if uright is None else np.ascontiguousarray(uright, np.float32)
        L.check(self.lib, self.lib.rgbl_device_frame_upload(self.h, len(d), L.ptr(d), L.ptr(a), L.ptr(o), L.ptr(u)))
        return self

    def capture(self, extractor, n, depth=None, frame=0, K=None, dist=None):
        """The n keypoints / descriptors of the extractor's last call (and the depth module's mvuRight): device to device."""
        k = None if K is None else np.ascontiguousarray(K, np.float32)
        dc = None if dist is None else np.ascontiguousarray(dist, np.float32).reshape(-1)
        L.check(self.lib, self.lib.rgbl_device_frame_capture(self.h, extractor.h, int(frame), int(n), depth.h if depth is not None else None,
                                                             L.ptr(k), L.ptr(dc), 0 if dc is None else len(dc)))
        return self

    def set_feature_vector(self, node_off, node_feat):
        off = np.ascontiguousarray(node_off, np.int32)
        ft = np.ascontiguousarray(node_feat, np.int32)
        L.check(self.lib, self.lib.rgbl_device_frame_set_feature_vector(self.h, len(off) - 1, L.ptr(off), L.ptr(ft) if len(ft) else None))
        return self

    def set_grid(self, grid):
        """Frame::AssignFeaturesToGrid kept with the frame (grid = mnMinX, mnMinY, mnMaxX, mnMaxY, the two inverse cell sizes)."""
        g = np.ascontiguousarray(grid, np.float32)
        L.check(self.lib, self.lib.rgbl_device_frame_set_grid(self.h, L.ptr(g)))
        return self

    def __len__(self):
        return self.lib.rgbl_device_frame_size(self.h)

    def download(self):
        n = len(self)
        desc, xy = np.zeros((n, 32), np.uint8), np.zeros((n, 2), np.float32)
        octave, ur = np.zeros(n, np.int32), np.zeros(n, np.float32)
        L.check(self.lib, self.lib.rgbl_device_frame_download(self.h, L.ptr(desc), L.ptr(xy), L.ptr(octave), L.ptr(ur)))
        return dict(desc=desc, xy=xy, octave=octave, uright=ur)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_device_frame_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dev(d, key):
    f = d.get(key) if hasattr(d, "get") else None
    return f.h if f is not None else None


class MapPointPool:
    """rgbl_map_points: what isInFrustum and the matcher read from the map points (GetWorldPos, GetNormal, mfMinDistance,
    mfMaxDistance, GetDescriptor), resident on the device in caller-numbered slots of 64 bytes.  Thread-safe."""

    def __init__(self, capacity, device=0, lib=None):
        self.lib = lib or L.load()
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_map_points_create(device, int(capacity), C.byref(self.h)))

    def capacity(self):
        return self.lib.rgbl_map_points_capacity(self.h)

    def reserve(self, capacity):
        L.check(self.lib, self.lib.rgbl_map_points_reserve(self.h, int(capacity)))

    def update(self, slot, world_pos=None, normal=None, min_dist=None, max_dist=None, desc=None):
        """Entry k of every array that is given goes to slot[k]; a field that is None stays as it is."""
        slot = np.ascontiguousarray(slot, np.int32)
        a = [None if v is None else np.ascontiguousarray(v, dt) for v, dt in
             ((world_pos, np.float32), (normal, np.float32), (min_dist, np.float32), (max_dist, np.float32), (desc, np.uint8))]
        for v, per in zip(a, (3, 3, 1, 1, 32)):
            if v is not None and v.size != per * len(slot):
                raise ValueError("MapPointPool.update: an array does not hold one entry per slot")
        L.check(self.lib, self.lib.rgbl_map_points_update(self.h, len(slot), L.ptr(slot), *[L.ptr(v) for v in a]))

    def download(self, slots):
        """The slots' present values (test / debug aid): dict(world_pos, normal, min_dist, max_dist, desc)."""
        slot = np.ascontiguousarray(slots, np.int32)
        n = len(slot)
        r = dict(world_pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32),
                 max_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))
        L.check(self.lib, self.lib.rgbl_map_points_download(self.h, n, L.ptr(slot), *[L.ptr(r[k]) for k in
                                                            ("world_pos", "normal", "min_dist", "max_dist", "desc")]))
        return r

    def refresh_input(self, case, keep):
        """rgbl_map_refresh_input of a cases.make_map_refresh_case-style dict: slot, obs_off, obs_kf, obs_feat, ref_kf, ref_level,
        kf_frames (DeviceFrame or None per key frame), kf_center, kf_bad, scale_factors; optional new_world_pos (written to
        the slots first), do_normal, do_descriptor (default 1).  `keep` collects the arrays the struct points to."""
        def arr(key, dt):
            v = case.get(key)
            if v is None:
                return None
            keep.append(np.ascontiguousarray(v, dt))
            return L.ptr(keep[-1])
        P = L.MapRefreshInput()
        P.n_points = len(case["slot"])
        P.slot, P.world_pos = arr("slot", np.int32), arr("new_world_pos", np.float32)
        P.obs_off, P.obs_kf, P.obs_feat = arr("obs_off", np.int32), arr("obs_kf", np.int32), arr("obs_feat", np.int32)
        P.ref_kf, P.ref_level = arr("ref_kf", np.int32), arr("ref_level", np.int32)
        frames = case.get("kf_frames")
        P.n_kfs = len(case["kf_center"]) if frames is None else len(frames)
        if frames is not None:
            keep.append((C.c_void_p * max(len(frames), 1))(*[f.h.value if f is not None else None for f in frames]))
            P.kf_frame = C.cast(keep[-1], C.c_void_p)
        P.kf_center, P.kf_bad = arr("kf_center", np.float32), arr("kf_bad", np.uint8)
        P.scale_factors = arr("scale_factors", np.float32)
        P.n_levels = int(case.get("n_levels", len(case["scale_factors"]) if case.get("scale_factors") is not None else 0))
        P.do_normal, P.do_descriptor = int(case.get("do_normal", 1)), int(case.get("do_descriptor", 1))
        return P

    def prepare_refresh(self, matcher, case):
        """MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors (MapPoint.cc:426-494, 329-403) of the listed slots
        from their observations in resident key frames, in one call on `matcher`'s stream.  The call returns
        dict(normal, min_dist, max_dist, best_obs, desc, status): the slots' values afterwards."""
        keep = []
        P = self.refresh_input(case, keep)
        n = P.n_points
        r = dict(normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32), max_dist=np.zeros(n, np.float32),
                 best_obs=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8), status=np.zeros(n, np.uint8))
        out = L.MapRefreshOutput(*[L.ptr(r[k]) for k in ("normal", "min_dist", "max_dist", "best_obs", "desc", "status")])
        fn, mh, ph, pP, pO = self.lib.rgbl_map_points_refresh, matcher.h, self.h, C.byref(P), C.byref(out)

        def call(_keep=keep):
            L.check(self.lib, fn(mh, ph, pP, pO))
            return r
        return call

    def refresh(self, matcher, case):
        return self.prepare_refresh(matcher, case)()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_map_points_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ORBmatcher:
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30  # src/ORBmatcher.cc:35-37

    def __init__(self, nnratio=0.6, checkOri=True, device=0, lib=None):
        self.lib = lib or L.load()
        self.mfNNratio, self.mbCheckOrientation = nnratio, checkOri
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_matcher_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_matcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def DescriptorDistance(self, a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return self.lib.rgbl_descriptor_distance(L.ptr(a), L.ptr(b))

    def BruteForce(self, descA, descB):
        """best index / best distance / second-best distance of every row of A in B."""
        a = np.ascontiguousarray(descA, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(descB, np.uint8).reshape(-1, 32)
        bi = np.full(len(a), -1, np.int32)
        bd = np.full(len(a), 256, np.int32)
        sd = np.full(len(a), 256, np.int32)
        L.check(self.lib, self.lib.rgbl_hamming_bf(self.h, L.ptr(a), len(a), L.ptr(b), len(b), L.ptr(bi), L.ptr(bd), L.ptr(sd)))
        return bi, bd, sd

    def StereoFishEyeMatches(self, desc_left, mono_left, desc_right, mono_right):
        """Frame::ComputeStereoFishEyeMatches up to the triangulation: (mvLeftToRightMatch candidates, best, second distances)."""
        a = np.ascontiguousarray(desc_left, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(desc_right, np.uint8).reshape(-1, 32)
        l2r = np.full(len(a), -1, np.int32)
        bd = np.full(len(a), 256, np.int32)
        sd = np.full(len(a), 256, np.int32)
        L.check(self.lib, self.lib.rgbl_stereo_fisheye_matches(self.h, L.ptr(a), len(a), int(mono_left), L.ptr(b), len(b), int(mono_right),
                                                               L.ptr(l2r), L.ptr(bd), L.ptr(sd)))
        return l2r, bd, sd

    def fundamental(self, K1, K2, R12, t12):
        a = [np.ascontiguousarray(v, np.float32) for v in (K1, K2, R12, t12)]
        F = np.zeros(9, np.float32)
        self.lib.rgbl_fundamental(L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]), L.ptr(a[3]), L.ptr(F))
        return F

    def SearchByProjection(self, frames, th, bMono):
        return self.prepare_SearchByProjection(frames, th, bMono)()

    def prepare_SearchByProjection(self, frames, th, bMono):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1676-1887).
        (prepare_*: the input block is built once, the returned closure is the C call alone - what bench.py times.)
        frames: dict with the LastFrame arrays valid1, world_pos1, mp_desc1, mp_observed1, octave1, angle1, the CurrentFrame
        arrays kp2_xy, kp2_octave, kp2_angle, uright2, desc2, and grid[6], Tcw_q/Tcw_t, Tlw_q/Tlw_t, K[4], mb, mbf,
        scale_factors.  Returns (match2: LastFrame feature index per CurrentFrame feature or -1, nmatches)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.ProjectionInput()
        P.n1 = len(frames["valid1"])
        P.valid1, P.world_pos1 = arr(frames["valid1"], np.uint8), arr(frames["world_pos1"], np.float32)
        P.mp_desc1, P.mp_observed1 = arr(frames["mp_desc1"], np.uint8), arr(frames["mp_observed1"], np.uint8)
        P.octave1, P.angle1 = arr(frames["octave1"], np.int32), arr(frames["angle1"], np.float32)
        P.n2 = len(frames["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(frames["kp2_xy"], np.float32), arr(frames["kp2_octave"], np.int32)
        P.kp2_angle, P.uright2 = arr(frames["kp2_angle"], np.float32), arr(frames["uright2"], np.float32)
        P.desc2 = arr(frames["desc2"], np.uint8)
        for name, n in (("grid", 6), ("Tcw_q", 4), ("Tcw_t", 3), ("Tlw_q", 4), ("Tlw_t", 3), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(frames[name][i])
        P.mb, P.mbf = float(frames["mb"]), float(frames["mbf"])
        P.scale_factors = arr(frames["scale_factors"], np.float32)
        P.n_levels = len(frames["scale_factors"])
        P.th, P.mono, P.check_orientation = float(th), int(bMono), int(self.mbCheckOrientation)
        P.device2 = _dev(frames, "device2")
        match2 = np.zeros(P.n2, np.int32)
        n = C.c_int(0)
        fn, h, pP, pm, pn = self.lib.rgbl_search_by_projection, self.h, C.byref(P), L.ptr(match2), C.byref(n)

        def call(_keep=keep):   # the closure owns the input arrays
            L.check(self.lib, fn(h, pP, pm, pn))
            return match2, n.value
        return call

    @staticmethod
    def PredictScale(dist3D, mfMaxDistance, mfLogScaleFactor, mnScaleLevels):
        """MapPoint::PredictScale(currentDist, Frame*) (src/MapPoint.cc:531-546) for arrays: ceil(logf(max / dist) / logScale),
        clamped to the pyramid; logf is the C library's (what std::log(float) calls), not numpy's."""
        libm = C.CDLL("libm.so.6")
        libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
        d = np.asarray(dist3D, np.float32)
        ratio = np.asarray(mfMaxDistance, np.float32) / d
        lsf = np.float32(mfLogScaleFactor)
        out = np.zeros(len(d), np.int32)
        for i, r in enumerate(ratio):
            q = np.float32(libm.logf(float(r))) / lsf
            # a zero, infinite or NaN distance: the reference converts an infinite or NaN quotient to int, which gives INT_MIN
            # on x86-64 (cvttsd2si), i.e. level 0 after the clamp - what the oracle and the device's isInFrustum return too
            n = int(np.ceil(q)) if np.isfinite(q) else 0
            out[i] = min(max(n, 0), int(mnScaleLevels) - 1)
        return out

    def SearchByProjectionKeyFrame(self, kf, th, ORBdist):
        return self.prepare_SearchByProjectionKeyFrame(kf, th, ORBdist)()

    def prepare_SearchByProjectionKeyFrame(self, kf, th, ORBdist):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1889-2010), the matcher
        of Tracking::Relocalization.  kf: dict with the key-frame map point arrays valid1 (has a good map point that is not in
        sAlreadyFound and whose distance to the camera centre is inside its scale-invariance range), world_pos1, mp_desc1,
        level1 (PredictScale), angle1, the CurrentFrame arrays kp2_xy, kp2_octave, kp2_angle, desc2, occupied2, and grid[6],
        Tcw_q / Tcw_t, K[4], scale_factors.  Returns (match2: key-frame feature index per frame feature or -1, nmatches)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.KeyFrameProjectionInput()
        P.n1 = len(kf["valid1"])
        P.valid1, P.world_pos1 = arr(kf["valid1"], np.uint8), arr(kf["world_pos1"], np.float32)
        P.mp_desc1, P.level1, P.angle1 = arr(kf["mp_desc1"], np.uint8), arr(kf["level1"], np.int32), arr(kf["angle1"], np.float32)
        P.n2 = len(kf["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(kf["kp2_xy"], np.float32), arr(kf["kp2_octave"], np.int32)
        P.kp2_angle, P.desc2 = arr(kf["kp2_angle"], np.float32), arr(kf["desc2"], np.uint8)
        P.occupied2 = arr(kf["occupied2"], np.uint8)
        for name, n in (("grid", 6), ("Tcw_q", 4), ("Tcw_t", 3), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(kf[name][i])
        P.scale_factors = arr(kf["scale_factors"], np.float32)
        P.n_levels = len(kf["scale_factors"])
        P.th, P.orb_dist, P.check_orientation = float(th), int(ORBdist), int(self.mbCheckOrientation)
        P.device2 = _dev(kf, "device2")
        match2 = np.zeros(P.n2, np.int32)
        n = C.c_int(0)
        fn, h, pP, pm, pn = self.lib.rgbl_search_by_projection_keyframe, self.h, C.byref(P), L.ptr(match2), C.byref(n)

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pm, pn))
            return match2, n.value
        return call

    def FuseSearch(self, case, th=3.0):
        return self.prepare_FuseSearch(case, th)()

    def prepare_FuseSearch(self, case, th=3.0):
        """The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:1148-1338): for every candidate map point the
        key-frame feature it would be fused with (bestDist <= TH_LOW) or -1, and bestDist.  case: dict with valid1 (map point
        present, good, not yet in the key frame, inside its scale-invariance range, seen under less than 60 degrees),
        world_pos1, mp_desc1, level1 (PredictScale), the key-frame arrays kp2_xy, kp2_octave, uright2, desc2, and grid[6],
        Tcw_q / Tcw_t, K[4], bf, scale_factors, inv_level_sigma2."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.FuseInput()
        P.n1 = len(case["valid1"])
        P.valid1, P.world_pos1 = arr(case["valid1"], np.uint8), arr(case["world_pos1"], np.float32)
        P.mp_desc1, P.level1 = arr(case["mp_desc1"], np.uint8), arr(case["level1"], np.int32)
        P.n2 = len(case["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(case["kp2_xy"], np.float32), arr(case["kp2_octave"], np.int32)
        P.uright2, P.desc2 = arr(case["uright2"], np.float32), arr(case["desc2"], np.uint8)
        for name, n in (("grid", 6), ("Tcw_q", 4), ("Tcw_t", 3), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(case[name][i])
        P.bf = float(case["bf"])
        P.scale_factors, P.inv_level_sigma2 = arr(case["scale_factors"], np.float32), arr(case["inv_level_sigma2"], np.float32)
        P.n_levels = len(case["scale_factors"])
        P.th = float(th)
        P.device2 = _dev(case, "device2")
        best = np.zeros(P.n1, np.int32)
        dist = np.zeros(P.n1, np.int32)
        fn, h, pP, pb, pd = self.lib.rgbl_fuse_search, self.h, C.byref(P), L.ptr(best), L.ptr(dist)

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pb, pd))
            return best, dist
        return call

    def ComputeDistinctiveDescriptors(self, descriptor_lists):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403) for a batch: descriptor_lists = one [n_i, 32] uint8 array
        per map point (its observed descriptors in the reference's order).  Returns BestIdx per point (-1 for an empty list)."""
        off = np.zeros(len(descriptor_lists) + 1, np.int32)
        for i, d in enumerate(descriptor_lists):
            off[i + 1] = off[i] + len(d)
        desc = (np.concatenate([np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptor_lists])
                if off[-1] else np.zeros((0, 32), np.uint8))
        best = np.zeros(len(descriptor_lists), np.int32)
        L.check(self.lib, self.lib.rgbl_distinctive_descriptors(self.h, L.ptr(desc) if off[-1] else None, L.ptr(off),
                                                                len(descriptor_lists), L.ptr(best)))
        return best

    def ProjectSearch(self, case, th, proj_form, max_dist):
        return self.prepare_ProjectSearch(case, th, proj_form, max_dist)()

    def prepare_ProjectSearch(self, case, th, proj_form, max_dist):
        """The per-point search of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (proj_form 0, max_dist TH_LOW) and of both
        directions of SearchBySim3 (proj_form 1, max_dist TH_HIGH): case has valid1, cam_pos1 (points already in the key
        frame's camera frame), mp_desc1, level1, kp2_xy, kp2_octave, desc2, grid[6], K[4], scale_factors.
        Returns (best feature per point or -1, best distance)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.ProjectSearchInput()
        P.n1 = len(case["valid1"])
        P.valid1, P.cam_pos1 = arr(case["valid1"], np.uint8), arr(case["cam_pos1"], np.float32)
        P.mp_desc1, P.level1 = arr(case["mp_desc1"], np.uint8), arr(case["level1"], np.int32)
        P.n2 = len(case["kp2_xy"])
        P.kp2_xy, P.kp2_octave, P.desc2 = arr(case["kp2_xy"], np.float32), arr(case["kp2_octave"], np.int32), arr(case["desc2"], np.uint8)
        for name, n in (("grid", 6), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(case[name][i])
        P.scale_factors = arr(case["scale_factors"], np.float32)
        P.n_levels = len(case["scale_factors"])
        P.th, P.proj_form, P.max_dist = float(th), int(proj_form), int(max_dist)
        P.device2 = _dev(case, "device2")
        best = np.zeros(P.n1, np.int32)
        dist = np.zeros(P.n1, np.int32)
        fn, h, pP, pb, pd = self.lib.rgbl_project_search, self.h, C.byref(P), L.ptr(best), L.ptr(dist)

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pb, pd))
            return best, dist
        return call

    def SearchByProjectionSim3(self, case, matched2, th, proj_form, max_dist):
        return self.prepare_SearchByProjectionSim3(case, matched2, th, proj_form, max_dist)()

    def prepare_SearchByProjectionSim3(self, case, matched2, th, proj_form, max_dist):
        """The greedy search of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (proj_form 0) and of
        its vpPointsKFs overload (proj_form 2), max_dist = floor(TH_LOW * ratioHamming); case as for ProjectSearch, matched2 =
        vpMatched[i] != NULL on entry.  Returns (point index stored in vpMatched[i2] by the call or -1, nmatches)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.ProjectSearchInput()
        P.n1 = len(case["valid1"])
        P.valid1, P.cam_pos1 = arr(case["valid1"], np.uint8), arr(case["cam_pos1"], np.float32)
        P.mp_desc1, P.level1 = arr(case["mp_desc1"], np.uint8), arr(case["level1"], np.int32)
        P.n2 = len(case["kp2_xy"])
        P.kp2_xy, P.kp2_octave, P.desc2 = arr(case["kp2_xy"], np.float32), arr(case["kp2_octave"], np.int32), arr(case["desc2"], np.uint8)
        for name, n in (("grid", 6), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(case[name][i])
        P.scale_factors = arr(case["scale_factors"], np.float32)
        P.n_levels = len(case["scale_factors"])
        P.th, P.proj_form, P.max_dist = float(th), int(proj_form), int(max_dist)
        P.device2 = _dev(case, "device2")
        m2 = np.ascontiguousarray(matched2, np.uint8)
        match = np.zeros(P.n2, np.int32)
        n = C.c_int(0)
        fn, h, pP, pb, pm, pn = self.lib.rgbl_search_by_projection_sim3, self.h, C.byref(P), L.ptr(m2), L.ptr(match), C.byref(n)

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pb, pm, pn))
            return match, n.value
        return call

    def SearchLocalPoints(self, pts, th):
        """Tracking::SearchLocalPoints.  pts with the map points themselves (world_pos1 ..., or pool + slot1; cases.make_local_map_case):
        the isInFrustum loop and the matcher in one call (prepare_TrackLocalPoints) -> (in_view, records, nToMatch, match2, nmatches).
        pts with what the loop left in the MapPoints (proj1 ...; cases.make_local_points_case): the matcher alone -> (match2, nmatches)."""
        if "proj1" not in pts:
            return self.prepare_TrackLocalPoints(pts, th)()
        return self.prepare_SearchLocalPoints(pts, th)()

    def prepare_SearchLocalPoints(self, pts, th):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (ORBmatcher.cc:43-213), the call of
        Tracking::SearchLocalPoints.  pts: dict with the map point arrays valid1, proj1 [n,3] (mTrackProjX, mTrackProjY,
        mTrackProjXR), level1, view_cos1, mp_desc1, mp_observed1, the frame arrays kp2_xy, kp2_octave, uright2, desc2,
        blocked2, and grid[6], scale_factors.  Returns (match2: map point index per frame feature or -1, nmatches)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.LocalPointsInput()
        P.n1 = len(pts["valid1"])
        P.valid1, P.proj1, P.level1 = arr(pts["valid1"], np.uint8), arr(pts["proj1"], np.float32), arr(pts["level1"], np.int32)
        P.view_cos1, P.mp_desc1 = arr(pts["view_cos1"], np.float32), arr(pts["mp_desc1"], np.uint8)
        P.mp_observed1 = arr(pts["mp_observed1"], np.uint8)
        P.n2 = len(pts["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(pts["kp2_xy"], np.float32), arr(pts["kp2_octave"], np.int32)
        P.uright2, P.desc2, P.blocked2 = arr(pts["uright2"], np.float32), arr(pts["desc2"], np.uint8), arr(pts["blocked2"], np.uint8)
        for i in range(6):
            P.grid[i] = float(pts["grid"][i])
        P.scale_factors = arr(pts["scale_factors"], np.float32)
        P.n_levels = len(pts["scale_factors"])
        P.th, P.nnratio = float(th), float(self.mfNNratio)
        P.device2 = _dev(pts, "device2")
        match2 = np.zeros(P.n2, np.int32)
        n = C.c_int(0)
        fn, h, pP, pm, pn = self.lib.rgbl_search_local_points, self.h, C.byref(P), L.ptr(match2), C.byref(n)

        def call(_keep=keep):   # the closure owns the input arrays
            L.check(self.lib, fn(h, pP, pm, pn))
            return match2, n.value
        return call

    def _track_local_input(self, case, th, keep):
        """rgbl_track_local_input from a cases.make_local_map_case dict; with case["pool"] (a MapPointPool) and case["slot1"] the
        map points come from the pool's slots instead of the host arrays."""
        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.TrackLocalInput()
        pool = case.get("pool")
        if pool is not None:
            P.pool, P.slot1 = pool.h, arr(case["slot1"], np.int32)
            P.n1 = len(case["slot1"])
        else:
            P.n1 = len(case["world_pos1"])
            P.world_pos1, P.normal1 = arr(case["world_pos1"], np.float32), arr(case["normal1"], np.float32)
            P.min_dist1, P.max_dist1 = arr(case["min_dist1"], np.float32), arr(case["max_dist1"], np.float32)
            P.mp_desc1 = arr(case["mp_desc1"], np.uint8)
        if case.get("consider1") is not None:
            P.consider1 = arr(case["consider1"], np.uint8)
        P.mp_observed1 = arr(case["mp_observed1"], np.uint8)
        P.n2 = len(case["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(case["kp2_xy"], np.float32), arr(case["kp2_octave"], np.int32)
        P.uright2, P.desc2 = arr(case["uright2"], np.float32), arr(case["desc2"], np.uint8)
        if case.get("blocked2") is not None:
            P.blocked2 = arr(case["blocked2"], np.uint8)
        for name, n in (("grid", 6), ("Rcw", 9), ("tcw", 3), ("Ow", 3), ("K", 4)):
            for i in range(n):
                getattr(P, name)[i] = float(case[name][i])
        P.scale_factors = arr(case["scale_factors"], np.float32)
        P.n_levels = int(case.get("n_levels", len(case["scale_factors"])))
        P.th, P.nnratio = float(th), float(self.mfNNratio)
        P.device2 = _dev(case, "device2")
        P.mbf, P.log_scale_factor = float(case["mbf"]), float(case["log_scale_factor"])
        P.viewing_cos_limit = float(case["viewing_cos_limit"])
        P.far_points, P.th_far_points = int(case["far_points"]), float(case["th_far_points"])
        return P

    def FrustumCull(self, case):
        return self.prepare_FrustumCull(case)()

    def prepare_FrustumCull(self, case):
        """Frame::isInFrustum (Frame.cc:602-664) + MapPoint::PredictScale for every considered local map point, the loop of
        Tracking::SearchLocalPoints (Tracking.cc:3399-3420).  Returns (in_view uint8, records of _lib.FRUSTUM_DTYPE, nToMatch)."""
        keep = []
        P = self._track_local_input(case, 1.0, keep)
        in_view = np.zeros(P.n1, np.uint8)
        rec = np.zeros(P.n1, L.FRUSTUM_DTYPE)
        n = C.c_int(0)
        fn, h, pP, pv, pr, pn = self.lib.rgbl_frustum_cull, self.h, C.byref(P), L.ptr(in_view), L.ptr(rec), C.byref(n)

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pv, pr, pn))
            return in_view, rec, n.value
        return call

    def prepare_TrackLocalPoints(self, case, th, records=True):
        """Tracking::SearchLocalPoints from its isInFrustum loop on (Tracking.cc:3399-3448) in one call: the cull above and
        ORBmatcher::SearchByProjection(F, mvpLocalMapPoints, th, bFarPoints, thFarPoints) behind it.
        Returns (in_view, records, nToMatch, match2: map point index per frame feature or -1, nmatches)."""
        keep = []
        P = self._track_local_input(case, th, keep)
        in_view = np.zeros(P.n1, np.uint8)
        rec = np.zeros(P.n1, L.FRUSTUM_DTYPE) if records else None
        match2 = np.zeros(P.n2, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        fn, h, pP, pv, pr, pn, pm, pnm = (self.lib.rgbl_track_local_points, self.h, C.byref(P), L.ptr(in_view), L.ptr(rec), C.byref(n),
                                          L.ptr(match2), C.byref(nm))

        def call(_keep=keep):
            L.check(self.lib, fn(h, pP, pv, pr, pn, pm, pnm))
            return in_view, rec, n.value, match2, nm.value
        return call

    def SearchForInitialization(self, case, windowSize=100):
        return self.prepare_SearchForInitialization(case, windowSize)()

    def prepare_SearchForInitialization(self, case, windowSize=100):
        """(every call starts from the case's vbPrevMatched again)
        ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:648-763).
        case: dict with kp1_octave, kp1_angle, desc1, prev_matched [n1,2] (vbPrevMatched), kp2_xy, kp2_octave, kp2_angle,
        desc2, grid[6].  Returns (vnMatches12, the updated vbPrevMatched, nmatches)."""
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data
        P = L.InitializationInput()
        P.n1 = len(case["kp1_octave"])
        P.kp1_octave, P.kp1_angle = arr(case["kp1_octave"], np.int32), arr(case["kp1_angle"], np.float32)
        P.desc1 = arr(case["desc1"], np.uint8)
        P.n2 = len(case["kp2_xy"])
        P.kp2_xy, P.kp2_octave = arr(case["kp2_xy"], np.float32), arr(case["kp2_octave"], np.int32)
        P.kp2_angle, P.desc2 = arr(case["kp2_angle"], np.float32), arr(case["desc2"], np.uint8)
        for i in range(6):
            P.grid[i] = float(case["grid"][i])
        P.window_size, P.nnratio, P.check_orientation = int(windowSize), float(self.mfNNratio), int(self.mbCheckOrientation)
        prev0 = np.ascontiguousarray(case["prev_matched"], np.float32)
        prev = prev0.copy()
        m12 = np.zeros(P.n1, np.int32)
        n = C.c_int(0)
        fn, h, pP, pp, pm, pn = self.lib.rgbl_search_for_initialization, self.h, C.byref(P), L.ptr(prev), L.ptr(m12), C.byref(n)

        def call(_keep=keep):
            prev[:] = prev0
            L.check(self.lib, fn(h, pP, pp, pm, pn))
            return m12, prev, n.value
        return call

    @staticmethod
    def _view(kf, keep):
        v = L.KeyframeView()
        v.n = len(kf["desc"])
        for field, key, dt in (("desc", "desc", np.uint8), ("kp_xy", "xy", np.float32),
                               ("kp_octave", "octave", np.int32), ("kp_angle", "angle", np.float32),
                               ("uright", "uright", np.float32), ("has_mappoint", "has_mp", np.uint8),
                               ("node_id", "node_id", np.int32), ("node_off", "node_off", np.int32),
                               ("node_feat", "node_feat", np.int32)):
            a = np.ascontiguousarray(kf[key], dt)
            keep.append(a)
            setattr(v, field, a.ctypes.data)
        v.n_nodes = len(kf["node_id"])
        v.device = _dev(kf, "device")
        return v

    def SearchByBoW(self, kf, frame, Nleft=-1):
        return self.prepare_SearchByBoW(kf, frame, Nleft)()

    def prepare_SearchByBoW(self, kf, frame, Nleft=-1):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:223-425).  kf / frame: dicts as for
        SearchForTriangulation; kf["has_mp"] = map point present and not bad.  Nleft = F.Nleft: -1 for a single camera, else the
        frame's features from Nleft on are the right camera's (the two-camera branches, :298-326, :357-386).  Returns (per frame
        feature the key-frame feature whose map point it gets, or -1; nmatches)."""
        keep = []
        v1, v2 = self._view(kf, keep), self._view(frame, keep)
        m = np.full(v2.n, -1, np.int32)
        nm = C.c_int(0)
        fn, h, p1, p2, nl, r, o, pm, pn = (self.lib.rgbl_search_by_bow_rig, self.h, C.byref(v1), C.byref(v2), int(Nleft), float(self.mfNNratio),
                                           int(self.mbCheckOrientation), L.ptr(m), C.byref(nm))

        def call(_keep=keep):   # the closure owns the input arrays
            L.check(self.lib, fn(h, p1, p2, nl, r, o, pm, pn))
            return m, nm.value
        return call

    def SearchByBoWKeyFrames(self, kf1, kf2):
        return self.prepare_SearchByBoWKeyFrames(kf1, kf2)()

    def prepare_SearchByBoWKeyFrames(self, kf1, kf2):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:765-905).  kf1 / kf2: dicts as for
        SearchForTriangulation, has_mp = map point present and not bad, angle = mvKeysUn[].angle.  Returns (per kf1 feature the
        kf2 feature whose map point it gets, or -1; nmatches)."""
        keep = []
        v1, v2 = self._view(kf1, keep), self._view(kf2, keep)
        m = np.full(v1.n, -1, np.int32)
        nm = C.c_int(0)
        fn, h, p1, p2, r, o, pm, pn = (self.lib.rgbl_search_by_bow_keyframes, self.h, C.byref(v1), C.byref(v2), float(self.mfNNratio),
                                       int(self.mbCheckOrientation), L.ptr(m), C.byref(nm))

        def call(_keep=keep):
            L.check(self.lib, fn(h, p1, p2, r, o, pm, pn))
            return m, nm.value
        return call

    def SearchForTriangulation(self, kf1, kf2, F12, ep, scale_factors2, level_sigma2_2, bOnlyStereo=False,
                               bCoarse=False):
        return self.prepare_SearchForTriangulation(kf1, kf2, F12, ep, scale_factors2, level_sigma2_2, bOnlyStereo, bCoarse)()

    def prepare_SearchForTriangulation(self, kf1, kf2, F12, ep, scale_factors2, level_sigma2_2, bOnlyStereo=False,
                                       bCoarse=False):
        """kf = dict(desc, xy, octave, angle, uright, has_mp, node_id, node_off, node_feat).
        Returns (vMatchedPairs as [m,2] int array in ascending idx1, nmatches)."""
        keep = []
        v1, v2 = self._view(kf1, keep), self._view(kf2, keep)
        P = L.TriangulationParams()
        for i in range(9):
            P.F12[i] = float(F12[i])
        P.epipole[0], P.epipole[1] = float(ep[0]), float(ep[1])
        sf = np.ascontiguousarray(scale_factors2, np.float32)
        s2 = np.ascontiguousarray(level_sigma2_2, np.float32)
        P.scale_factors2, P.level_sigma2_2, P.n_levels = sf.ctypes.data, s2.ctypes.data, len(sf)
        P.only_stereo, P.coarse, P.check_orientation = int(bOnlyStereo), int(bCoarse), int(self.mbCheckOrientation)
        m12 = np.full(v1.n, -1, np.int32)
        nm = C.c_int(0)
        keep += [sf, s2]
        fn, h, p1, p2, pP, pm, pn = self.lib.rgbl_search_triangulation, self.h, C.byref(v1), C.byref(v2), C.byref(P), L.ptr(m12), C.byref(nm)

        def call(_keep=keep):   # the closure owns the input arrays
            L.check(self.lib, fn(h, p1, p2, pP, pm, pn))
            idx1 = np.nonzero(m12 >= 0)[0]
            pairs = np.stack([idx1, m12[idx1]], 1) if len(idx1) else np.zeros((0, 2), np.int64)
            return pairs, nm.value, m12
        return call

    @staticmethod
    def _new_points_kf(kf, keep, out=None):
        """rgbl_new_points_keyframe of a key-frame dict: the keys of SearchForTriangulation plus depth (mvDepth), xy_raw
        (mvKeys[].pt, optional), Tcw (3 x 4), Ow, K (fx, fy, cx, cy), mb, mbf, scale_factors, level_sigma2."""
        k = out if out is not None else L.NewPointsKeyframe()
        k.view = ORBmatcher._view(kf, keep)
        for field, key in (("depth", "depth"), ("kp_xy_raw", "xy_raw"), ("scale_factors", "scale_factors"),
                           ("level_sigma2", "level_sigma2")):
            if kf.get(key) is None:
                setattr(k, field, None)
                continue
            a = np.ascontiguousarray(kf[key], np.float32)
            keep.append(a)
            setattr(k, field, a.ctypes.data)
        for field, key, cnt in (("Tcw", "Tcw", 12), ("Ow", "Ow", 3), ("K", "K", 4)):
            v = np.asarray(kf[key], np.float32).reshape(-1)
            for i in range(cnt):
                getattr(k, field)[i] = float(v[i])
        k.mb, k.mbf = float(kf["mb"]), float(kf["mbf"])
        return k

    @staticmethod
    def _new_points_params(prm):
        P = L.NewPointsParams()
        P.n_levels, P.ratio_factor = int(prm["n_levels"]), float(prm["ratio_factor"])
        P.far_points, P.th_far_points = int(prm.get("far_points", 0)), float(prm.get("th_far_points", 0.0))
        P.inertial, P.monocular = int(prm.get("inertial", 0)), int(prm.get("monocular", 0))
        P.report_rejected = int(prm.get("report_rejected", 0))
        return P

    def TriangulateMatches(self, kf1, kf2, prm, idx1, idx2, host=False):
        """The per-match block of LocalMapping::CreateNewMapPoints (LocalMapping.cc:481-691) on explicit pairs: one record
        (L.NEW_POINT_DTYPE) per pair.  host=True: the same header evaluated by the library's host build (no device)."""
        keep = []
        k1, k2, P = self._new_points_kf(kf1, keep), self._new_points_kf(kf2, keep), self._new_points_params(prm)
        i1, i2 = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
        out = np.zeros(len(i1), L.NEW_POINT_DTYPE)
        if host:
            rc = self.lib.rgbl_triangulate_matches_host(C.byref(k1), C.byref(k2), C.byref(P), len(i1), L.ptr(i1), L.ptr(i2), L.ptr(out))
        else:
            rc = self.lib.rgbl_triangulate_matches(self.h, C.byref(k1), C.byref(k2), C.byref(P), len(i1), L.ptr(i1), L.ptr(i2), L.ptr(out))
        L.check(self.lib, rc)
        return out

    @staticmethod
    def _pose_opt_input(fr, keep, out=None):
        """rgbl_pose_opt_input of a frame dict: mp_index (per feature, -1 = none), world_pos (points x 3) or pool (MapPointPool)
        + slot, xy / octave / uright or device (DeviceFrame), q (x y z w), t, K (fx fy cx cy), bf, inv_level_sigma2."""
        P = out if out is not None else L.PoseOptInput()

        def arr(key, dt):
            if fr.get(key) is None:
                return None
            keep.append(np.ascontiguousarray(fr[key], dt))
            return keep[-1].ctypes.data
        mp = np.ascontiguousarray(fr["mp_index"], np.int32)
        keep.append(mp)
        P.n, P.mp_index = len(mp), mp.ctypes.data
        pool = fr.get("pool")
        P.pool = pool.h if pool is not None else None
        P.world_pos, P.slot = arr("world_pos", np.float32), arr("slot", np.int32)
        P.n_points = int(fr["n_points"]) if fr.get("n_points") is not None else (
            len(fr["slot"]) if pool is not None else len(np.asarray(fr["world_pos"]).reshape(-1, 3)))
        P.kp_xy, P.kp_octave, P.uright = arr("xy", np.float32), arr("octave", np.int32), arr("uright", np.float32)
        P.device = _dev(fr, "device")
        for field, key, cnt in (("Tcw_q", "q", 4), ("Tcw_t", "t", 3), ("K", "K", 4)):
            v = np.asarray(fr[key], np.float32).reshape(-1)
            for i in range(cnt):
                getattr(P, field)[i] = v[i]
        P.bf = np.float32(fr["bf"])
        P.inv_level_sigma2 = arr("inv_level_sigma2", np.float32)
        P.n_levels = int(fr.get("n_levels", len(fr["inv_level_sigma2"])))
        return P

    @staticmethod
    def _pose_opt_result(O, outlier):
        d = O.diag
        return dict(q=np.array(O.Tcw_q, np.float32), t=np.array(O.Tcw_t, np.float32), outlier=outlier, result=int(O.result),
                    rounds=int(d.rounds), iterations=np.array(d.iterations, np.int32), active=np.array(d.active, np.int32),
                    chi2=np.array(d.chi2, np.float64), q64=np.array(d.Tcw_q, np.float64), t64=np.array(d.Tcw_t, np.float64))

    def prepare_PoseOptimizationBatch(self, frames, host=False, outlier_fill=0):
        """Optimizer::PoseOptimization (Optimizer.cc:814-1114) of every frame dict in one launch; the call returns one dict per
        frame: q, t (what SetPose receives), outlier (mvbOutlier, `outlier_fill` where there is no map point), result (the
        reference's return value) and the diagnostics rounds / iterations / active / chi2."""
        keep = []
        B = len(frames)
        I, O = (L.PoseOptInput * max(B, 1))(), (L.PoseOptOutput * max(B, 1))()
        outl = []
        for b, fr in enumerate(frames):
            self._pose_opt_input(fr, keep, I[b])
            outl.append(np.full(I[b].n, outlier_fill, np.uint8))
            O[b].outlier = outl[b].ctypes.data
        lib, h = self.lib, self.h

        def call(_keep=keep):
            if host:
                for b in range(B):
                    L.check(lib, lib.rgbl_pose_optimization_host(C.byref(I[b]), C.byref(O[b])))
            else:
                L.check(lib, lib.rgbl_pose_optimization_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
            return [self._pose_opt_result(O[b], outl[b]) for b in range(B)]

        def c_call(_keep=keep):   # the C call alone (what tools/pose_opt_bench.py times): the results stay in the structs
            L.check(lib, lib.rgbl_pose_optimization_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
        call.c_call = c_call
        return call

    def PoseOptimizationBatch(self, frames, host=False, outlier_fill=0):
        return self.prepare_PoseOptimizationBatch(frames, host, outlier_fill)()

    def PoseOptimization(self, frame, host=False, outlier_fill=0):
        """One frame through rgbl_pose_optimization (host=True: rgbl_pose_optimization_host, the header's host build)."""
        keep = []
        I, O = self._pose_opt_input(frame, keep), L.PoseOptOutput()
        outl = np.full(I.n, outlier_fill, np.uint8)
        O.outlier = outl.ctypes.data
        if host:
            L.check(self.lib, self.lib.rgbl_pose_optimization_host(C.byref(I), C.byref(O)))
        else:
            L.check(self.lib, self.lib.rgbl_pose_optimization(self.h, C.byref(I), C.byref(O)))
        return self._pose_opt_result(O, outl)

    @staticmethod
    def _sim3_input(pr, keep, out=None):
        """rgbl_sim3_input of a problem dict: x1c / x2c (n x 3 camera frames) or pool (MapPointPool) + slot1 / slot2 + Rcw1, tcw1,
        Rcw2, tcw2; max_err1, max_err2, K1, K2 (fx fy cx cy), fix_scale, min_inliers, best_inliers (default 0), samples (n_hyp x 3)."""
        P = out if out is not None else L.Sim3Input()

        def arr(key, dt):
            if pr.get(key) is None:
                return None
            keep.append(np.ascontiguousarray(pr[key], dt))
            return keep[-1].ctypes.data
        pool = pr.get("pool")
        P.pool = pool.h if pool is not None else None
        P.x1c, P.x2c = arr("x1c", np.float32), arr("x2c", np.float32)
        P.slot1, P.slot2 = arr("slot1", np.int32), arr("slot2", np.int32)
        P.max_err1, P.max_err2 = arr("max_err1", np.float32), arr("max_err2", np.float32)
        P.n = int(pr["n"]) if pr.get("n") is not None else len(np.asarray(pr["max_err1"]).reshape(-1))
        for field, cnt in (("Rcw1", 9), ("tcw1", 3), ("Rcw2", 9), ("tcw2", 3), ("K1", 4), ("K2", 4)):
            if pr.get(field) is None:
                continue
            v = np.asarray(pr[field], np.float32).reshape(-1)
            for i in range(cnt):
                getattr(P, field)[i] = v[i]
        P.fix_scale, P.min_inliers, P.best_inliers = int(pr["fix_scale"]), int(pr["min_inliers"]), int(pr.get("best_inliers", 0))
        P.samples = arr("samples", np.int32)
        P.n_hyp = int(pr["n_hyp"]) if pr.get("n_hyp") is not None else (0 if pr.get("samples") is None else len(np.asarray(pr["samples"]).reshape(-1, 3)))
        return P

    @staticmethod
    def _sim3_buffers(I, O, fill=0, diag=True):
        """the caller's arrays of one rgbl_sim3_output, pre-filled with `fill` so that what a call leaves untouched can be seen"""
        inl = np.full(I.n, fill, np.uint8)
        counts = np.full(I.n_hyp, fill, np.int32) if diag else None
        T_all = np.full((I.n_hyp, 16), fill, np.float32) if diag else None
        O.inlier = inl.ctypes.data
        O.counts = counts.ctypes.data if diag else None
        O.T12_all = T_all.ctypes.data if diag else None
        return inl, counts, T_all

    @staticmethod
    def _sim3_result(O, bufs):
        inl, counts, T_all = bufs
        return dict(selected=int(O.selected), converged=int(O.converged), n_inliers=int(O.n_inliers), iterations_run=int(O.iterations_run),
                    T12=np.array(O.T12, np.float32).reshape(4, 4), R12=np.array(O.R12, np.float32).reshape(3, 3),
                    t12=np.array(O.t12, np.float32), s12=np.float32(O.s12), inlier=inl, counts=counts, T12_all=T_all)

    def prepare_Sim3RansacBatch(self, problems, host=False, diag=True, fill=0):
        """Sim3Solver (Sim3Solver.cc) for every problem dict in one upload, one launch pair and one read-back; the call returns
        one dict per problem: selected, converged, n_inliers, iterations_run, T12 (4 x 4), R12, t12, s12, inlier (n bytes) and,
        with diag, counts (n_hyp) and T12_all (n_hyp x 16).  With selected = -1 the transformation and the flags are not
        written; for a problem that is not run (n < 3, n < min_inliers, no hypothesis) nothing but selected is."""
        keep = []
        B = len(problems)
        I, O = (L.Sim3Input * max(B, 1))(), (L.Sim3Output * max(B, 1))()
        bufs = []
        for b, pr in enumerate(problems):
            self._sim3_input(pr, keep, I[b])
            bufs.append(self._sim3_buffers(I[b], O[b], fill, diag))
        lib, h = self.lib, self.h

        def call(_keep=keep):
            if host:
                for b in range(B):
                    L.check(lib, lib.rgbl_sim3_ransac_host(C.byref(I[b]), C.byref(O[b])))
            else:
                L.check(lib, lib.rgbl_sim3_ransac_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
            return [self._sim3_result(O[b], bufs[b]) for b in range(B)]

        def c_call(_keep=keep):   # the C call alone (what tools/sim3_bench.py times): the results stay in the structs
            L.check(lib, lib.rgbl_sim3_ransac_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))

        def c_call_host(_keep=keep):
            for b in range(B):
                L.check(lib, lib.rgbl_sim3_ransac_host(C.byref(I[b]), C.byref(O[b])))
        call.c_call, call.c_call_host = c_call, c_call_host
        return call

    def Sim3RansacBatch(self, problems, host=False, diag=True, fill=0):
        return self.prepare_Sim3RansacBatch(problems, host, diag, fill)()

    def Sim3Ransac(self, problem, host=False, diag=True, fill=0):
        """One problem through rgbl_sim3_ransac (host=True: rgbl_sim3_ransac_host, the header's host build)."""
        keep = []
        I, O = self._sim3_input(problem, keep), L.Sim3Output()
        bufs = self._sim3_buffers(I, O, fill, diag)
        if host:
            L.check(self.lib, self.lib.rgbl_sim3_ransac_host(C.byref(I), C.byref(O)))
        else:
            L.check(self.lib, self.lib.rgbl_sim3_ransac(self.h, C.byref(I), C.byref(O)))
        return self._sim3_result(O, bufs)

    @staticmethod
    def _mlpnp_input(pr, keep, out=None):
        """rgbl_mlpnp_input of a problem dict: mp_index (per feature, -1 = none), world_pos (points x 3) or pool (MapPointPool) +
        slot, xy / octave or device (DeviceFrame), K (fx fy cx cy), level_sigma2, th2, min_inliers (after SetRansacParameters),
        best_inliers / best_mask (N bytes) / best_Tcw (the state of earlier calls; default: a fresh solver), samples (n_hyp x 6)."""
        P = out if out is not None else L.MlpnpInput()

        def arr(key, dt):
            if pr.get(key) is None:
                return None
            keep.append(np.ascontiguousarray(pr[key], dt))
            return keep[-1].ctypes.data
        P.mp_index = arr("mp_index", np.int32)
        P.n = int(pr["n"]) if pr.get("n") is not None else len(np.asarray(pr["mp_index"]).reshape(-1))
        pool = pr.get("pool")
        P.pool = pool.h if pool is not None else None
        P.world_pos, P.slot = arr("world_pos", np.float32), arr("slot", np.int32)
        P.n_points = int(pr["n_points"]) if pr.get("n_points") is not None else (
            len(pr["slot"]) if pool is not None else len(np.asarray(pr["world_pos"]).reshape(-1, 3)))
        P.kp_xy, P.kp_octave = arr("xy", np.float32), arr("octave", np.int32)
        P.device = _dev(pr, "device")
        K = np.asarray(pr["K"], np.float32).reshape(-1)
        for i in range(4):
            P.K[i] = K[i]
        P.level_sigma2 = arr("level_sigma2", np.float32)
        P.n_levels = int(pr["n_levels"]) if pr.get("n_levels") is not None else len(pr["level_sigma2"])
        P.th2 = np.float32(pr["th2"])
        P.min_inliers, P.best_inliers = int(pr["min_inliers"]), int(pr.get("best_inliers", 0))
        P.best_mask = arr("best_mask", np.uint8)
        T = np.asarray(pr["best_Tcw"] if pr.get("best_Tcw") is not None else np.eye(4), np.float32).reshape(-1)
        for i in range(16):
            P.best_Tcw[i] = T[i]
        P.samples = arr("samples", np.int32)
        P.n_hyp = int(pr["n_hyp"]) if pr.get("n_hyp") is not None else (0 if pr.get("samples") is None else len(np.asarray(pr["samples"]).reshape(-1, 6)))
        return P

    @staticmethod
    def _mlpnp_buffers(I, O, fill=0, diag=True):
        """the caller's arrays of one rgbl_mlpnp_output, pre-filled with `fill` so that what a call leaves untouched can be seen"""
        nh = max(I.n_hyp, 0)
        inl, best = np.full(max(I.n, 0), fill, np.uint8), np.full(max(I.n, 0), fill, np.uint8)
        counts = np.full(nh, fill, np.int32) if diag else None
        T_all = np.full((nh, 3, 4), fill, np.float64) if diag else None
        path = np.full(nh, fill, np.int32) if diag else None
        O.inlier, O.best_mask = inl.ctypes.data, best.ctypes.data
        O.counts = counts.ctypes.data if diag else None
        O.Tcw_all = T_all.ctypes.data if diag else None
        O.gn_path = path.ctypes.data if diag else None
        return inl, best, counts, T_all, path

    @staticmethod
    def _mlpnp_result(O, bufs):
        inl, best, counts, T_all, path = bufs
        return dict(found=int(O.found), no_more=int(O.no_more), n_inliers=int(O.n_inliers), iterations_run=int(O.iterations_run),
                    Tcw=np.array(O.Tcw, np.float32).reshape(4, 4), inlier=inl, best_inliers=int(O.best_inliers), best_mask=best,
                    best_Tcw=np.array(O.best_Tcw, np.float32).reshape(4, 4), refines=int(O.refines), counts=counts, Tcw_all=T_all,
                    gn_path=path)

    def prepare_MLPnPRansacBatch(self, problems, host=False, diag=True, fill=0):
        """MLPnPsolver::iterate (MLPnPsolver.cpp:100-223) for every problem dict in one upload, one launch pair and one read-back;
        the call returns one dict per problem: found, no_more, n_inliers, iterations_run, Tcw (4 x 4), inlier (n bytes per
        feature, written when found), the new state best_inliers / best_mask (the first N of its n bytes, per correspondence) /
        best_Tcw, refines and, with diag, counts (n_hyp), Tcw_all (n_hyp x 3 x 4, fp64) and gn_path (n_hyp)."""
        keep = []
        B = len(problems)
        I, O = (L.MlpnpInput * max(B, 1))(), (L.MlpnpOutput * max(B, 1))()
        bufs = []
        for b, pr in enumerate(problems):
            self._mlpnp_input(pr, keep, I[b])
            bufs.append(self._mlpnp_buffers(I[b], O[b], fill, diag))
        lib, h = self.lib, self.h

        def call(_keep=keep):
            if host:
                for b in range(B):
                    L.check(lib, lib.rgbl_mlpnp_ransac_host(C.byref(I[b]), C.byref(O[b])))
            else:
                L.check(lib, lib.rgbl_mlpnp_ransac_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
            return [self._mlpnp_result(O[b], bufs[b]) for b in range(B)]

        def c_call(_keep=keep):   # the C call alone (what tools/mlpnp_bench.py times): the results stay in the structs
            L.check(lib, lib.rgbl_mlpnp_ransac_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))

        def c_call_host(_keep=keep):
            for b in range(B):
                L.check(lib, lib.rgbl_mlpnp_ransac_host(C.byref(I[b]), C.byref(O[b])))
        call.c_call, call.c_call_host = c_call, c_call_host
        return call

    def MLPnPRansacBatch(self, problems, host=False, diag=True, fill=0):
        return self.prepare_MLPnPRansacBatch(problems, host, diag, fill)()

    def MLPnPRansac(self, problem, host=False, diag=True, fill=0):
        """One problem through rgbl_mlpnp_ransac (host=True: rgbl_mlpnp_ransac_host, the header's host build)."""
        keep = []
        I, O = self._mlpnp_input(problem, keep), L.MlpnpOutput()
        bufs = self._mlpnp_buffers(I, O, fill, diag)
        if host:
            L.check(self.lib, self.lib.rgbl_mlpnp_ransac_host(C.byref(I), C.byref(O)))
        else:
            L.check(self.lib, self.lib.rgbl_mlpnp_ransac(self.h, C.byref(I), C.byref(O)))
        return self._mlpnp_result(O, bufs)

    @staticmethod
    def _two_view_input(pr, keep, out=None):
        """rgbl_two_view_input of a problem dict: xy1 / xy2 (keys x 2) or device1 / device2 (DeviceFrame) with n1 / n2,
        matches12 (n1 entries, -1 = none), K (fx fy cx cy), sigma, samples (n_hyp x 8 indices into the matches)."""
        P = out if out is not None else L.TwoViewInput()

        def arr(key, dt):
            if pr.get(key) is None:
                return None
            keep.append(np.ascontiguousarray(pr[key], dt))
            return keep[-1].ctypes.data
        P.matches12 = arr("matches12", np.int32)
        P.kp1_xy, P.kp2_xy = arr("xy1", np.float32), arr("xy2", np.float32)
        P.device1, P.device2 = _dev(pr, "device1"), _dev(pr, "device2")
        P.n1 = int(pr["n1"]) if pr.get("n1") is not None else len(np.asarray(pr["matches12"]).reshape(-1))
        P.n2 = int(pr["n2"]) if pr.get("n2") is not None else len(np.asarray(pr["xy2"]).reshape(-1, 2))
        K = np.asarray(pr["K"], np.float32).reshape(-1)
        for i in range(4):
            P.K[i] = K[i]
        P.sigma = np.float32(pr.get("sigma", 1.0))
        P.samples = arr("samples", np.int32)
        P.n_hyp = int(pr["n_hyp"]) if pr.get("n_hyp") is not None else (0 if pr.get("samples") is None else len(np.asarray(pr["samples"]).reshape(-1, 8)))
        return P

    @staticmethod
    def _two_view_buffers(I, O, fill=0, diag=True):
        """the caller's arrays of one rgbl_two_view_output, pre-filled with `fill` so that what a call leaves untouched can be seen"""
        n1, nh = max(I.n1, 0), max(I.n_hyp, 0)
        p3d, tri = np.full((n1, 3), fill, np.float32), np.full(n1, fill, np.uint8)
        O.p3d, O.triangulated = p3d.ctypes.data, tri.ctypes.data
        scores = np.full((nh, 2), fill, np.float32) if diag else None
        models = np.full((nh, 2, 3, 3), fill, np.float32) if diag else None
        inl_h = np.full(n1, fill, np.uint8) if diag else None     # N <= n1 bytes are written
        inl_f = np.full(n1, fill, np.uint8) if diag else None
        O.scores = scores.ctypes.data if diag else None
        O.models = models.ctypes.data if diag else None
        O.inliers_h = inl_h.ctypes.data if diag else None
        O.inliers_f = inl_f.ctypes.data if diag else None
        return p3d, tri, scores, models, inl_h, inl_f

    @staticmethod
    def _two_view_result(O, bufs):
        p3d, tri, scores, models, inl_h, inl_f = bufs
        return dict(found=int(O.found), model=int(O.model), exit_code=int(O.exit_code), SH=np.float32(O.SH), SF=np.float32(O.SF),
                    best_h=int(O.best_h), best_f=int(O.best_f), H21=np.array(O.H21, np.float32).reshape(3, 3),
                    F21=np.array(O.F21, np.float32).reshape(3, 3), R21=np.array(O.R21, np.float32).reshape(3, 3),
                    t21=np.array(O.t21, np.float32), p3d=p3d, triangulated=tri, p3d_assigned=int(O.p3d_assigned),
                    n_inliers=int(O.n_inliers), best_motion=int(O.best_motion), aux=int(O.aux), n_good=np.array(O.n_good, np.int32),
                    parallax=np.array(O.parallax, np.float32), scores=scores, models=models, inliers_h=inl_h, inliers_f=inl_f)

    def prepare_TwoViewReconstructBatch(self, problems, host=False, diag=True, fill=0):
        """TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:41-129) for every problem dict in one upload, one launch
        sequence and one read-back; the call returns one dict per problem: found, model (0 H, 1 F, -1 none), exit_code, SH, SF,
        best_h, best_f, H21, F21, R21, t21, p3d (n1 x 3) and triangulated (n1), both written when found, p3d_assigned, n_inliers,
        best_motion, aux, n_good (8), parallax (8) and, with diag, scores (n_hyp x 2), models (n_hyp x 2 x 3 x 3), inliers_h and
        inliers_f (the first N of their n1 bytes, per match)."""
        keep = []
        B = len(problems)
        I, O = (L.TwoViewInput * max(B, 1))(), (L.TwoViewOutput * max(B, 1))()
        bufs = []
        for b, pr in enumerate(problems):
            self._two_view_input(pr, keep, I[b])
            bufs.append(self._two_view_buffers(I[b], O[b], fill, diag))
        lib, h = self.lib, self.h

        def call(_keep=keep):
            if host:
                for b in range(B):
                    L.check(lib, lib.rgbl_two_view_reconstruct_host(C.byref(I[b]), C.byref(O[b])))
            else:
                L.check(lib, lib.rgbl_two_view_reconstruct_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
            return [self._two_view_result(O[b], bufs[b]) for b in range(B)]

        def c_call(_keep=keep):   # the C call alone (what tools/two_view_bench.py times): the results stay in the structs
            L.check(lib, lib.rgbl_two_view_reconstruct_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))

        def c_call_host(_keep=keep):
            for b in range(B):
                L.check(lib, lib.rgbl_two_view_reconstruct_host(C.byref(I[b]), C.byref(O[b])))
        call.c_call, call.c_call_host = c_call, c_call_host
        return call

    def TwoViewReconstructBatch(self, problems, host=False, diag=True, fill=0):
        return self.prepare_TwoViewReconstructBatch(problems, host, diag, fill)()

    def TwoViewReconstruct(self, problem, host=False, diag=True, fill=0):
        """One problem through rgbl_two_view_reconstruct (host=True: rgbl_two_view_reconstruct_host, the header's host build)."""
        keep = []
        I, O = self._two_view_input(problem, keep), L.TwoViewOutput()
        bufs = self._two_view_buffers(I, O, fill, diag)
        if host:
            L.check(self.lib, self.lib.rgbl_two_view_reconstruct_host(C.byref(I), C.byref(O)))
        else:
            L.check(self.lib, self.lib.rgbl_two_view_reconstruct(self.h, C.byref(I), C.byref(O)))
        return self._two_view_result(O, bufs)

    @staticmethod
    def _sim3_opt_input(cs, keep, out=None):
        """rgbl_sim3_opt_input of a case dict: mp1_index, match_index, i2, track_level2 (per feature of key frame 1), bad and
        world_pos (points x 3) or pool (MapPointPool) + slot, Rcw1, tcw1, Rcw2, tcw2, xy1 / octave1 or device1 (DeviceFrame),
        xy2 / octave2 or device2, inv_level_sigma2_1 / _2, K1, K2, the entry estimate R (3 x 3; or q, x y z w), t, s, th2,
        fix_scale, all_points.  R becomes a quaternion as g2o::Sim3(Matrix3d, ...) makes it (LoopClosing.cc:746)."""
        P = out if out is not None else L.Sim3OptInput()

        def arr(key, dt):
            if cs.get(key) is None:
                return None
            keep.append(np.ascontiguousarray(cs[key], dt))
            return keep[-1].ctypes.data
        P.mp1_index, P.match_index = arr("mp1_index", np.int32), arr("match_index", np.int32)
        P.i2, P.track_level2 = arr("i2", np.int32), arr("track_level2", np.int32)
        P.n = int(cs["n"]) if cs.get("n") is not None else len(np.asarray(cs["match_index"]).reshape(-1))
        pool = cs.get("pool")
        P.pool = pool.h if pool is not None else None
        P.bad, P.world_pos, P.slot = arr("bad", np.uint8), arr("world_pos", np.float32), arr("slot", np.int32)
        P.n_points = int(cs["n_points"]) if cs.get("n_points") is not None else len(np.asarray(cs["bad"]).reshape(-1))
        P.kp1_xy, P.kp1_octave = arr("xy1", np.float32), arr("octave1", np.int32)
        P.kp2_xy, P.kp2_octave = arr("xy2", np.float32), arr("octave2", np.int32)
        P.device1, P.device2 = _dev(cs, "device1"), _dev(cs, "device2")
        P.n2 = int(cs["n2"])
        P.inv_level_sigma2_1, P.inv_level_sigma2_2 = arr("inv_level_sigma2_1", np.float32), arr("inv_level_sigma2_2", np.float32)
        P.n_levels1 = int(cs.get("n_levels1", len(cs["inv_level_sigma2_1"])))
        P.n_levels2 = int(cs.get("n_levels2", len(cs["inv_level_sigma2_2"])))
        for field, cnt in (("Rcw1", 9), ("tcw1", 3), ("Rcw2", 9), ("tcw2", 3), ("K1", 4), ("K2", 4)):
            v = np.asarray(cs[field], np.float32).reshape(-1)
            for i in range(cnt):
                getattr(P, field)[i] = v[i]
        q = np.asarray(cs["q"], np.float64) if cs.get("q") is not None else quat_from_matrix(cs["R"])
        t = np.asarray(cs["t"], np.float64)
        for i in range(4):
            P.q[i] = q[i]
        for i in range(3):
            P.t[i] = t[i]
        P.s, P.th2 = float(cs["s"]), np.float32(cs["th2"])
        P.fix_scale, P.all_points = int(cs["fix_scale"]), int(cs["all_points"])
        return P

    @staticmethod
    def _sim3_opt_result(O, cleared):
        d = O.diag
        out = dict(result=int(O.result), q=np.array(O.q, np.float64), t=np.array(O.t, np.float64), s=float(O.s), cleared=cleared,
                   iterations=np.array(d.iterations, np.int32), active=np.array(d.active, np.int32),
                   chi2=np.array(d.chi2, np.float64), rounds=int(d.rounds))
        for k in ("n_correspondences", "n_bad_mps", "n_in_kf2", "n_out_kf2", "n_without_mp", "n_bad"):
            out[k] = int(getattr(d, k))
        return out

    def prepare_OptimizeSim3Batch(self, problems, host=False, cleared_fill=0):
        """Optimizer::OptimizeSim3 (Optimizer.cc:2115-2381) of every case dict in one upload, one launch and one read-back; the
        call returns one dict per problem: result (nIn, or 0), q (x y z w) / t / s (g2oS12 on return), cleared (n bytes, 1 where
        vpMatches1[i] becomes NULL, `cleared_fill` where no edge pair existed), the counters of the set-up loop and the
        diagnostics n_bad / iterations / active / chi2 / rounds."""
        keep = []
        B = len(problems)
        I, O = (L.Sim3OptInput * max(B, 1))(), (L.Sim3OptOutput * max(B, 1))()
        clr = []
        for b, cs in enumerate(problems):
            self._sim3_opt_input(cs, keep, I[b])
            clr.append(np.full(I[b].n, cleared_fill, np.uint8))
            O[b].cleared = clr[b].ctypes.data
        lib, h = self.lib, self.h

        def call(_keep=keep):
            if host:
                for b in range(B):
                    L.check(lib, lib.rgbl_optimize_sim3_host(C.byref(I[b]), C.byref(O[b])))
            else:
                L.check(lib, lib.rgbl_optimize_sim3_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))
            return [self._sim3_opt_result(O[b], clr[b]) for b in range(B)]

        def c_call(_keep=keep):   # the C call alone (what tools/sim3_opt_bench.py times): the results stay in the structs
            L.check(lib, lib.rgbl_optimize_sim3_batch(h, B, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)))

        def c_call_host(_keep=keep):
            for b in range(B):
                L.check(lib, lib.rgbl_optimize_sim3_host(C.byref(I[b]), C.byref(O[b])))
        call.c_call, call.c_call_host = c_call, c_call_host
        return call

    def OptimizeSim3Batch(self, problems, host=False, cleared_fill=0):
        return self.prepare_OptimizeSim3Batch(problems, host, cleared_fill)()

    def OptimizeSim3(self, case, host=False, cleared_fill=0):
        """One candidate through rgbl_optimize_sim3 (host=True: rgbl_optimize_sim3_host, the header's host build)."""
        keep = []
        I, O = self._sim3_opt_input(case, keep), L.Sim3OptOutput()
        clr = np.full(I.n, cleared_fill, np.uint8)
        O.cleared = clr.ctypes.data
        if host:
            L.check(self.lib, self.lib.rgbl_optimize_sim3_host(C.byref(I), C.byref(O)))
        else:
            L.check(self.lib, self.lib.rgbl_optimize_sim3(self.h, C.byref(I), C.byref(O)))
        return self._sim3_opt_result(O, clr)

    def LocalBundleAdjustment(self, case, host=False, fill=0):
        """Optimizer::LocalBundleAdjustment from :1188 on through rgbl_local_bundle_adjustment (host=True: the header's host
        build, no device).  case: an lba_cases.make_lba_case-style dict (local_bundle_adjustment_call lists its keys)."""
        return local_bundle_adjustment_call(self.lib, None if host else self.h, case, fill)()

    def prepare_LocalBundleAdjustment(self, case, fill=0):
        return local_bundle_adjustment_call(self.lib, self.h, case, fill)

    def BundleAdjustment(self, case, host=False, fill=0):
        """Optimizer::BundleAdjustment's optimize(nIterations) (Optimizer.cc:281) through rgbl_bundle_adjustment (host=True: the
        header's host build, no device).  case: an lba_cases.make_ba_case-style dict (bundle_adjustment_call lists its keys)."""
        return bundle_adjustment_call(self.lib, None if host else self.h, case, fill)()

    def prepare_BundleAdjustment(self, case, fill=0):
        return bundle_adjustment_call(self.lib, self.h, case, fill)

    def CreateNewMapPoints(self, kf1, neighbours, prm, skip=None, cap=None):
        return self.prepare_CreateNewMapPoints(kf1, neighbours, prm, skip, cap)()

    def prepare_CreateNewMapPoints(self, kf1, neighbours, prm, skip=None, cap=None):
        """LocalMapping::CreateNewMapPoints from its neighbour loop on (LocalMapping.cc:434-711) in one call.
        kf1: key-frame dict (see _new_points_kf); neighbours: list of dict(kf=key-frame dict, F12=, ep=, coarse=, only_stereo=)
        in the order of vpNeighKFs; prm: dict(n_levels, ratio_factor, far_points, th_far_points, inertial, monocular,
        report_rejected); skip: per neighbour, the caller's monocular median-depth test.  Returns (records, matches per
        neighbour with -1 for one left out, kf1's has_mp after the call)."""
        keep = []
        k1, P = self._new_points_kf(kf1, keep), self._new_points_params(prm)
        nn = len(neighbours)
        k2 = (L.NewPointsKeyframe * max(nn, 1))()
        tp = (L.TriangulationParams * max(nn, 1))()
        for i, nb in enumerate(neighbours):
            self._new_points_kf(nb["kf"], keep, k2[i])
            for j in range(9):
                tp[i].F12[j] = float(nb["F12"][j])
            tp[i].epipole[0], tp[i].epipole[1] = float(nb["ep"][0]), float(nb["ep"][1])
            tp[i].scale_factors2, tp[i].level_sigma2_2, tp[i].n_levels = k2[i].scale_factors, k2[i].level_sigma2, P.n_levels
            tp[i].only_stereo, tp[i].coarse = int(nb.get("only_stereo", 0)), int(nb.get("coarse", 0))
            tp[i].check_orientation = int(self.mbCheckOrientation)
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        n1 = k1.view.n
        cap = n1 if cap is None else int(cap)
        out = np.zeros(max(cap, 1), L.NEW_POINT_DTYPE)
        per = np.zeros(max(nn, 1), np.int32)
        mask = np.ascontiguousarray(kf1["has_mp"], np.uint8).copy()
        n_out = C.c_int(0)
        fn, h = self.lib.rgbl_create_new_map_points, self.h
        args = (h, C.byref(k1), nn, C.cast(k2, C.c_void_p), C.cast(tp, C.c_void_p), L.ptr(sk), C.byref(P), L.ptr(out), cap,
                C.byref(n_out), L.ptr(per), L.ptr(mask))

        def call(_keep=(keep, k2, tp, sk)):   # the closure owns the input arrays
            L.check(self.lib, fn(*args))
            return out[:n_out.value], per[:nn], mask
        call.out, call.mask = out, mask   # what an error return must leave untouched (tests)
        return call

    @staticmethod
    def new_points_left_out(kf1, neighbours, prm, skip, i):
        """LocalMapping.cc:444-460 for neighbour i: the caller's skip[], or (not monocular) a baseline below pKF2->mb, in fp32"""
        if skip is not None and skip[i]:
            return True
        if prm.get("monocular", 0):
            return False
        kf2 = neighbours[i]["kf"]
        d = np.asarray(kf2["Ow"], np.float32) - np.asarray(kf1["Ow"], np.float32)
        sq = np.float32(d[0] * d[0])
        sq = np.float32(sq + np.float32(d[1] * d[1]))
        sq = np.float32(sq + np.float32(d[2] * d[2]))
        return bool(np.float32(np.sqrt(sq)) < np.float32(kf2["mb"]))

    def CreateNewMapPointsRestatement(self, search, kf1, neighbours, prm, skip=None, chained=True, block=None):
        """The loop of LocalMapping.cc:434-711 restated neighbour by neighbour on the host: search(kf1 with the mask so far, nb)
        -> matches12 is SearchForTriangulation (the tests hand in the oracle's, tools/new_points_bench.py the device's single
        call), then the per-match block by the host build of csrc/newpoint_math.h (block(i, idx1, idx2) -> records; default
        TriangulateMatches(host=True)), then the has_mappoint feedback of :701.  chained=False: every neighbour searches with
        the mask the call started from.  Returns what CreateNewMapPoints returns."""
        mask = np.ascontiguousarray(kf1["has_mp"], np.uint8).copy()
        start = mask.copy()
        if block is None:
            def block(i, idx1, idx2):
                return self.TriangulateMatches(kf1, neighbours[i]["kf"], prm, idx1, idx2, host=True)
        recs, per = [], []
        for i, nb in enumerate(neighbours):
            if self.new_points_left_out(kf1, neighbours, prm, skip, i):
                per.append(-1)
                continue
            m12 = search(dict(kf1, has_mp=mask.copy() if chained else start), nb)
            idx1 = np.nonzero(m12 >= 0)[0].astype(np.int32)
            r = block(i, idx1, np.ascontiguousarray(m12[idx1], np.int32))
            r["neighbour"] = i
            acc = (r["status"] >= 1) & (r["status"] <= 3)
            mask[idx1[acc]] = 1
            recs.append((r if prm.get("report_rejected", 0) else r[acc]).copy())
            per.append(len(idx1))
        recs = np.concatenate(recs) if recs else np.zeros(0, L.NEW_POINT_DTYPE)
        return recs, np.array(per, np.int32), mask

    def profile(self, enable):
        L.check(self.lib, self.lib.rgbl_matcher_profile(self.h, int(enable)))

    def profile_read(self):
        return L.read_profile(self.lib, self.lib.rgbl_matcher_profile_read, self.h)

    def profile_samples(self):
        return L.read_profile_samples(self.lib, self.lib.rgbl_matcher_profile_read, self.lib.rgbl_matcher_profile_samples, self.h)


class ORBVocabulary:
    """DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h) on the device: loadFromTextFile +
    transform(features, BowVector, FeatureVector, levelsup) as Frame::ComputeBoW calls it (src/Frame.cc:828-835)."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or L.load()
        self.device = device
        self.h = C.c_void_p()

    def loadFromTextFile(self, path):
        self.close()
        rc = self.lib.rgbl_vocabulary_load_text(str(path).encode(), self.device, C.byref(self.h))
        if rc != L.RGBL_OK:
            self.h = C.c_void_p()
            return False
        return True

    def from_arrays(self, arrays):
        """arrays: synth.vocabulary_arrays(...) layout (n_nodes, L, child_off, child, desc, weight, word_id)."""
        self.close()
        keep = [np.ascontiguousarray(arrays[k]) for k in ("child_off", "child", "desc", "weight", "word_id")]
        L.check(self.lib, self.lib.rgbl_vocabulary_create(arrays["n_nodes"], arrays["L"], *[L.ptr(a) for a in keep], self.device,
                                                          C.byref(self.h)))
        return self

    def info(self):
        k, lv, nn, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.check(self.lib, self.lib.rgbl_vocabulary_info(self.h, C.byref(k), C.byref(lv), C.byref(nn), C.byref(nw)))
        return dict(k=k.value, L=lv.value, n_nodes=nn.value, n_words=nw.value)

    def transform(self, features, levelsup=4):
        return self.prepare_transform(features, levelsup)()

    def prepare_transform(self, features, levelsup=4):
        """features: [n, 32] u8.  Returns (BowVector word ids, BowVector values, FeatureVector node ids, node offsets,
        feature indices)."""
        desc = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(desc)
        wid, wval = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        nid, noff, nfeat = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(0), C.c_int(0)
        args = (self.h, L.ptr(desc), n, levelsup, L.ptr(wid), L.ptr(wval), n, C.byref(nw), L.ptr(nid), L.ptr(noff), L.ptr(nfeat), n,
                C.byref(nn))

        def call():
            L.check(self.lib, self.lib.rgbl_bow_transform(*args))
            return wid[:nw.value].copy(), wval[:nw.value].copy(), nid[:nn.value].copy(), noff[:nn.value + 1].copy(), nfeat[:noff[nn.value]].copy()
        return call

    def prepare_transform_frame(self, frame, levelsup=4):
        """transform() of a DeviceFrame's resident descriptors: nothing is uploaded."""
        n = len(frame)
        wid, wval = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        nid, noff, nfeat = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(0), C.c_int(0)
        args = (self.h, frame.h, levelsup, L.ptr(wid), L.ptr(wval), n, C.byref(nw), L.ptr(nid), L.ptr(noff), L.ptr(nfeat), n, C.byref(nn))

        def call():
            L.check(self.lib, self.lib.rgbl_bow_transform_frame(*args))
            return wid[:nw.value].copy(), wval[:nw.value].copy(), nid[:nn.value].copy(), noff[:nn.value + 1].copy(), nfeat[:noff[nn.value]].copy()
        return call

    def close(self):
        if self.h:
            self.lib.rgbl_vocabulary_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyFrameDatabase:
    """ORB_SLAM3::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) with the stored BowVectors on the
    device: add / erase / clear / clearMap, the BoW part of a query (`query`), and the two Detect* functions the reference
    calls, whose covisibility tail runs here on plain arrays, in float32 like the reference's `float` locals.

    Key frames are integers.  The stamps the reference keeps on the KeyFrame objects (mnRelocQuery / mnRelocWords /
    mRelocScore and the mnPlaceRecognition* trio) are kept in `self.stamps`; a score that was never written reads 0 (the
    reference leaves mRelocScore uninitialised).  Query ids are taken to differ from 0 and from every earlier query's, as
    Frame::mnId / KeyFrame::mnId of the reference's callers do."""

    def __init__(self, n_vocab_words, device=0, lib=None):
        self.lib = lib or L.load()
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_kfdb_create(device, int(n_vocab_words), C.byref(self.h)))
        self.stamps = {"reloc": {}, "place": {}}

    def close(self):
        if self.h:
            self.lib.rgbl_kfdb_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, kf_id, map_id, word_id, word_val):
        wid, wval = np.ascontiguousarray(word_id, np.uint32), np.ascontiguousarray(word_val, np.float64)
        L.check(self.lib, self.lib.rgbl_kfdb_add(self.h, int(kf_id), int(map_id), len(wid), L.ptr(wid), L.ptr(wval)))

    def erase(self, kf_id):
        L.check(self.lib, self.lib.rgbl_kfdb_erase(self.h, int(kf_id)))

    def clear(self):
        L.check(self.lib, self.lib.rgbl_kfdb_clear(self.h))

    def clearMap(self, map_id):
        L.check(self.lib, self.lib.rgbl_kfdb_clear_map(self.h, int(map_id)))

    def setMap(self, kf_id, map_id):
        """KeyFrame::UpdateMap of a stored key frame: clearMap goes by the map a key frame has when it runs."""
        L.check(self.lib, self.lib.rgbl_kfdb_set_map(self.h, int(kf_id), int(map_id)))

    def size(self):
        n, w = C.c_int(0), C.c_longlong(0)
        L.check(self.lib, self.lib.rgbl_kfdb_size(self.h, C.byref(n), C.byref(w)))
        return n.value, w.value

    def arena_info(self):
        used, cap, slots, comp = C.c_longlong(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
        L.check(self.lib, self.lib.rgbl_kfdb_arena_info(self.h, C.byref(used), C.byref(cap), C.byref(slots), C.byref(comp)))
        return dict(used_words=used.value, cap_words=cap.value, n_slots=slots.value, n_compactions=comp.value)

    def query(self, word_id, word_val, excluded=None, min_words_floor=0, cap=None):
        return self.prepare_query(word_id, word_val, excluded, min_words_floor, cap)()

    def prepare_query(self, word_id, word_val, excluded=None, min_words_floor=0, cap=None):
        """lKFsSharingWords of one query through rgbl_kfdb_query: dict(kf, words, score, scored, max_common_words,
        min_common_words); score is meaningful where scored."""
        wid, wval = np.ascontiguousarray(word_id, np.uint32), np.ascontiguousarray(word_val, np.float64)
        ex = np.ascontiguousarray([] if excluded is None else sorted(excluded), np.int64)
        cap = self.arena_info()["n_slots"] if cap is None else int(cap)
        kf, words = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
        score, scored = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.uint8)
        qin = L.KfdbQueryInput(len(wid), L.ptr(wid).value, L.ptr(wval).value, len(ex), L.ptr(ex).value if len(ex) else None,
                               int(min_words_floor))
        out = L.KfdbQueryOutput(cap, L.ptr(kf).value, L.ptr(words).value, L.ptr(score).value, L.ptr(scored).value, 0, 0, 0)
        keep = (wid, wval, ex)

        def call():
            L.check(self.lib, self.lib.rgbl_kfdb_query(self.h, C.byref(qin), C.byref(out)))
            n = out.n_share
            assert keep is not None
            return dict(kf=kf[:n].copy(), words=words[:n].copy(), score=score[:n].copy(), scored=scored[:n].astype(bool),
                        max_common_words=out.max_common_words, min_common_words=out.min_common_words)
        return call

    def query_batch(self, queries, cap=None):
        return self.prepare_query_batch(queries, cap)()

    def prepare_query_batch(self, queries, cap=None):
        """queries: a list of dict(word_id, word_val[, excluded][, min_words_floor]); one rgbl_kfdb_query_batch call.
        Returns one result dict per query, as `query` does."""
        Q = len(queries)
        off = np.zeros(Q + 1, np.int32)
        xoff = np.zeros(Q + 1, np.int32)
        for i, q in enumerate(queries):
            off[i + 1] = off[i] + len(q["word_id"])
            xoff[i + 1] = xoff[i] + len(q.get("excluded") or ())
        wid = np.ascontiguousarray(np.concatenate([np.asarray(q["word_id"], np.uint32) for q in queries] + [np.zeros(0, np.uint32)]))
        wval = np.ascontiguousarray(np.concatenate([np.asarray(q["word_val"], np.float64) for q in queries] + [np.zeros(0, np.float64)]))
        ex = np.ascontiguousarray(np.concatenate([np.asarray(sorted(q.get("excluded") or ()), np.int64) for q in queries] + [np.zeros(0, np.int64)]))
        floor = np.ascontiguousarray([int(q.get("min_words_floor", 0)) for q in queries], np.int32)
        cap = self.arena_info()["n_slots"] if cap is None else int(cap)
        c1 = max(cap, 1)
        kf, words = np.zeros((Q, c1), np.int64), np.zeros((Q, c1), np.int32)
        score, scored = np.zeros((Q, c1), np.float32), np.zeros((Q, c1), np.uint8)
        ns, mx, mn = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
        if cap == 0:
            kf, words, score, scored = kf[:, :0], words[:, :0], score[:, :0], scored[:, :0]
        args = (self.h, Q, L.ptr(off), L.ptr(wid), L.ptr(wval), L.ptr(xoff) if xoff[Q] else None, L.ptr(ex), L.ptr(floor), c1 if cap else 0,
                L.ptr(kf), L.ptr(words), L.ptr(score), L.ptr(scored), L.ptr(ns), L.ptr(mx), L.ptr(mn))

        def call():
            L.check(self.lib, self.lib.rgbl_kfdb_query_batch(*args))
            return [dict(kf=kf[i, :ns[i]].copy(), words=words[i, :ns[i]].copy(), score=score[i, :ns[i]].copy(),
                         scored=scored[i, :ns[i]].astype(bool), max_common_words=int(mx[i]), min_common_words=int(mn[i]))
                    for i in range(Q)]
        return call

    def profile(self, enable):
        L.check(self.lib, self.lib.rgbl_kfdb_profile(self.h, int(enable)))

    def profile_read(self):
        return L.read_profile(self.lib, self.lib.rgbl_kfdb_profile_read, self.h)

    # ---- the host tails (KeyFrameDatabase.cc:671-729, :792-844)
    def _stamp(self, which, query_id, r):
        st = self.stamps[which]
        scored = []
        for kf, w, s, ok in zip(r["kf"].tolist(), r["words"].tolist(), r["score"], r["scored"].tolist()):
            e = st.setdefault(kf, [0, 0, np.float32(0)])
            e[0], e[1] = query_id, w
            if ok:
                e[2] = np.float32(s)
                scored.append((np.float32(s), kf))
        return st, scored

    @staticmethod
    def _accumulate(st, scored, query_id, covisibility):
        acc_list, best_acc = [], np.float32(0)
        for si, kf in scored:
            best, acc, best_kf = si, si, kf
            for kf2 in list(covisibility.get(kf, ()))[:10]:     # GetBestCovisibilityKeyFrames(10)
                e2 = st.get(kf2)
                if e2 is None or e2[0] != query_id:
                    continue
                acc = np.float32(acc + e2[2])
                if e2[2] > best:
                    best_kf, best = kf2, e2[2]
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return acc_list, best_acc

    def DetectRelocalizationCandidates(self, frame_id, word_id, word_val, map_id, covisibility, kf_map):
        """KeyFrameDatabase::DetectRelocalizationCandidates(F, pMap) (:733-845).  covisibility: {kf: its covisible key
        frames, best first}; kf_map: {kf: map id}.  Returns vpRelocCandidates."""
        r = self.query(word_id, word_val)
        st, scored = self._stamp("reloc", frame_id, r)
        if not scored:
            return []
        acc_list, best_acc = self._accumulate(st, scored, frame_id, covisibility)
        min_retain = np.float32(np.float32(0.75) * best_acc)
        out, seen = [], set()
        for si, kf in acc_list:
            if si > min_retain:
                if kf_map[kf] != map_id:
                    continue
                if kf not in seen:
                    out.append(kf)
                    seen.add(kf)
        return out

    def DetectNBestCandidates(self, kf_id, word_id, word_val, map_id, connected, nNumCandidates, covisibility, kf_map,
                              bad_kfs=(), bad_maps=()):
        """KeyFrameDatabase::DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) (:604-730); connected =
        pKF->GetConnectedKeyFrames().  Returns (vpLoopCand, vpMergeCand).  A bad key frame in the sorted list is stepped
        over (the reference's `continue` at :712 does not advance and would spin; bad key frames are erased from the database
        before they can be met, KeyFrame.cc:678)."""
        r = self.query(word_id, word_val, excluded=connected)
        st, scored = self._stamp("place", kf_id, r)
        if not scored:
            return [], []
        acc_list, _ = self._accumulate(st, scored, kf_id, covisibility)
        acc_list = sorted(acc_list, key=lambda p: -float(p[0]))   # list::sort(compFirst): stable, descending
        loop, merge, seen = [], [], set()
        bad_kfs, bad_maps = set(bad_kfs), set(bad_maps)
        for _, kf in acc_list:
            if not (len(loop) < nNumCandidates or len(merge) < nNumCandidates):
                break
            if kf in bad_kfs:
                continue
            if kf not in seen:
                if map_id == kf_map[kf] and len(loop) < nNumCandidates:
                    loop.append(kf)
                elif map_id != kf_map[kf] and len(merge) < nNumCandidates and kf_map[kf] not in bad_maps:
                    merge.append(kf)
                seen.add(kf)
        return loop, merge

def frustum_terms(case):
    """The float32 intermediates of isInFrustum for every point, in the reference's order: Pc (x, y, z), invz, u, v, |Pc|,
    dist = |P - Ow|, viewCos, ratio = mfMaxDistance / dist."""
    f = np.float32
    P = np.ascontiguousarray(case["world_pos1"], f).reshape(-1, 3)
    Pn = np.ascontiguousarray(case["normal1"], f).reshape(-1, 3)
    R, t, Ow, K = [np.asarray(case[k], f) for k in ("Rcw", "tcw", "Ow", "K")]
    with np.errstate(all="ignore"):
        p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]

        def row(k):
            return ((R[3 * k] * p0 + R[3 * k + 1] * p1) + R[3 * k + 2] * p2) + t[k]
        x, y, z = row(0), row(1), row(2)

        def norm(a, b, c):
            return np.sqrt((a * a + b * b) + c * c)
        o0, o1, o2 = p0 - Ow[0], p1 - Ow[1], p2 - Ow[2]
        dist = norm(o0, o1, o2)
        return dict(x=x, y=y, z=z, invz=f(1) / z, u=(K[0] * x) / z + K[2], v=(K[1] * y) / z + K[3], pc_dist=norm(x, y, z), dist=dist,
                    view_cos=((o0 * Pn[:, 0] + o1 * Pn[:, 1]) + o2 * Pn[:, 2]) / dist, ratio=np.asarray(case["max_dist1"], f) / dist)


def frustum_restatement(case):
    """Frame::isInFrustum (src/Frame.cc:602-664, single camera) + MapPoint::PredictScale (src/MapPoint.cc:531-546) for the
    points of a cases.make_local_map_case dict, in numpy float32 in the reference's order (three-term sums left to right, as
    csrc/frustum_math.h) with the C library's logf.  Returns (in_view uint8, records of _lib.FRUSTUM_DTYPE, stage): stage 0 =
    not considered, 1 .. 4 = rejected by depth / image bounds / distance / viewing angle, 5 = in view."""
    f = np.float32
    n1 = len(case["world_pos1"])
    consider = np.ones(n1, bool) if case.get("consider1") is None else np.asarray(case["consider1"]) != 0
    minX, minY, maxX, maxY = [f(v) for v in np.asarray(case["grid"], f)[:4]]
    rec = np.zeros(n1, L.FRUSTUM_DTYPE)
    rec["proj_x"] = -1
    rec["proj_y"] = -1
    stage = np.zeros(n1, np.int32)
    if n1 == 0:
        return np.zeros(0, np.uint8), rec, stage
    with np.errstate(all="ignore"):
        T = frustum_terms(case)
        z, u, v, invz, pc_dist, dist, view_cos, ratio = [T[k] for k in ("z", "u", "v", "invz", "pc_dist", "dist", "view_cos", "ratio")]
        max_d, min_d = f(1.2) * np.asarray(case["max_dist1"], f), f(0.8) * np.asarray(case["min_dist1"], f)
        r1 = z < f(0)
        r2 = (u < minX) | (u > maxX) | (v < minY) | (v > maxY)
        r3 = (dist < min_d) | (dist > max_d)
        r4 = view_cos < f(case["viewing_cos_limit"])
        stage[:] = np.where(r1, 1, np.where(r2, 2, np.where(r3, 3, np.where(r4, 4, 5))))
        stage[~consider] = 0
        keep_uv = stage >= 3
        rec["proj_x"][keep_uv] = u[keep_uv]
        rec["proj_y"][keep_uv] = v[keep_uv]
        seen = stage == 5
        rec["proj_xr"][seen] = (u - f(case["mbf"]) * invz)[seen]
        rec["depth"][seen] = pc_dist[seen]
        rec["view_cos"][seen] = view_cos[seen]
        libm = C.CDLL("libm.so.6")
        libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
        lsf, n_levels = f(case["log_scale_factor"]), int(case.get("n_levels", len(case["scale_factors"])))
        for i in np.nonzero(seen)[0]:
            r = ratio[i]
            level = 0
            if r > 0 and np.isfinite(r):   # else: the reference's float -> int conversion is undefined; the device says 0
                c = np.ceil(f(libm.logf(float(r))) / lsf)
                level = 0 if not c >= 0 else (n_levels - 1 if c >= n_levels else int(c))
            rec["level"][i] = level
    return seen.astype(np.uint8), rec, stage


def pose_optimization_host(frame, lib=None, outlier_fill=0):
    """rgbl_pose_optimization_host: Optimizer::PoseOptimization by the host build of csrc/poseopt_math.h (no device, no handle);
    the result dict of ORBmatcher.PoseOptimization."""
    lib = lib or L.load()
    keep = []
    I, O = ORBmatcher._pose_opt_input(frame, keep), L.PoseOptOutput()
    outl = np.full(I.n, outlier_fill, np.uint8)
    O.outlier = outl.ctypes.data
    L.check(lib, lib.rgbl_pose_optimization_host(C.byref(I), C.byref(O)))
    return ORBmatcher._pose_opt_result(O, outl)


def sim3_ransac_host(problem, lib=None, diag=True, fill=0):
    """rgbl_sim3_ransac_host: Sim3Solver by the host build of csrc/sim3_math.h (no device, no handle); the result dict of
    ORBmatcher.Sim3Ransac."""
    lib = lib or L.load()
    keep = []
    I, O = ORBmatcher._sim3_input(problem, keep), L.Sim3Output()
    bufs = ORBmatcher._sim3_buffers(I, O, fill, diag)
    L.check(lib, lib.rgbl_sim3_ransac_host(C.byref(I), C.byref(O)))
    return ORBmatcher._sim3_result(O, bufs)


def mlpnp_ransac_host(problem, lib=None, diag=True, fill=0):
    """rgbl_mlpnp_ransac_host: MLPnPsolver by the host build of csrc/mlpnp_math.h (no device, no handle); the result dict of
    ORBmatcher.MLPnPRansac."""
    lib = lib or L.load()
    keep = []
    I, O = ORBmatcher._mlpnp_input(problem, keep), L.MlpnpOutput()
    bufs = ORBmatcher._mlpnp_buffers(I, O, fill, diag)
    L.check(lib, lib.rgbl_mlpnp_ransac_host(C.byref(I), C.byref(O)))
    return ORBmatcher._mlpnp_result(O, bufs)


def quat_from_matrix(R):
    """Quaterniond(Matrix3d) as Eigen assigns it, in the arithmetic of csrc/poseopt_math.h (po_quat_from_matrix): x y z w"""
    m = np.asarray(R, np.float64).reshape(9)
    q = np.zeros(4, np.float64)
    t = (m[0] + m[4]) + m[8]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
    elif not m[4] > m[0] and not m[8] > m[0]:
        t = np.sqrt(((m[0] - m[4]) - m[8]) + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[3], q[1], q[2] = (m[7] - m[5]) * t, (m[3] + m[1]) * t, (m[6] + m[2]) * t
    elif m[4] > m[0] and not m[8] > m[4]:
        t = np.sqrt(((m[4] - m[8]) - m[0]) + 1.0)
        q[1] = 0.5 * t
        t = 0.5 / t
        q[3], q[2], q[0] = (m[2] - m[6]) * t, (m[7] + m[5]) * t, (m[1] + m[3]) * t
    else:
        t = np.sqrt(((m[8] - m[0]) - m[4]) + 1.0)
        q[2] = 0.5 * t
        t = 0.5 / t
        q[3], q[0], q[1] = (m[3] - m[1]) * t, (m[2] + m[6]) * t, (m[5] + m[7]) * t
    return q


def optimize_sim3_host(case, lib=None, cleared_fill=0):
    """rgbl_optimize_sim3_host: Optimizer::OptimizeSim3 by the host build of csrc/sim3opt_math.h (no device, no handle); the
    result dict of ORBmatcher.OptimizeSim3."""
    lib = lib or L.load()
    keep = []
    I, O = ORBmatcher._sim3_opt_input(case, keep), L.Sim3OptOutput()
    clr = np.full(I.n, cleared_fill, np.uint8)
    O.cleared = clr.ctypes.data
    L.check(lib, lib.rgbl_optimize_sim3_host(C.byref(I), C.byref(O)))
    return ORBmatcher._sim3_opt_result(O, clr)


def local_bundle_adjustment_call(lib, handle, case, fill=0):
    """The call of rgbl_local_bundle_adjustment (handle None: rgbl_local_bundle_adjustment_host) on a case dict:
    n_free, n_fixed, free_is_fixed (optional), cam_q, cam_t, cam_K, cam_bf, world_pos (or pool = MapPointPool with slot),
    edge_point, edge_cam, edge_obs, edge_inv_sigma2; optional max_iterations (10), user_lambda_init (0), stop (an int32 array
    of one element), stop_byte (a uint8 array of one element) and stop_after_polls (0).  Every output array starts as `fill` bytes, so a test sees what a call left
    untouched.  Returns a callable that gives dict(cam_q, cam_t, point, chi2, flags, q, t, X (the estimates in double) and
    the diag's scalars); its .outputs holds the raw arrays."""
    def arr(key, dt):
        v = case.get(key)
        return None if v is None else np.ascontiguousarray(v, dt)
    nf, nx = int(case["n_free"]), int(case["n_fixed"])
    a = dict(free_is_fixed=arr("free_is_fixed", np.uint8), cam_q=arr("cam_q", np.float32), cam_t=arr("cam_t", np.float32),
             cam_K=arr("cam_K", np.float32), cam_bf=arr("cam_bf", np.float32), world_pos=arr("world_pos", np.float32),
             slot=arr("slot", np.int32), edge_point=arr("edge_point", np.int32), edge_cam=arr("edge_cam", np.int32),
             edge_obs=arr("edge_obs", np.float32), edge_inv_sigma2=arr("edge_inv_sigma2", np.float32),
             stop=arr("stop", np.int32), stop_byte=arr("stop_byte", np.uint8))
    pool = case.get("pool")
    n_points = int(case["n_points"]) if "n_points" in case else (len(a["slot"]) if pool is not None else a["world_pos"].size // 3)
    n_edges = int(case["n_edges"]) if "n_edges" in case else (0 if a["edge_point"] is None else len(a["edge_point"]))
    I = L.LbaInput()
    I.n_free, I.n_fixed, I.n_points, I.n_edges = nf, nx, n_points, n_edges
    for k in ("free_is_fixed", "cam_q", "cam_t", "cam_K", "cam_bf", "slot", "edge_point", "edge_cam", "edge_obs",
              "edge_inv_sigma2", "stop", "stop_byte"):
        setattr(I, k, L.ptr(a[k]))
    I.world_pos = L.ptr(a["world_pos"]) if pool is None else None
    I.pool = pool.h if pool is not None else None
    I.max_iterations = int(case.get("max_iterations", 10))
    I.user_lambda_init = float(case.get("user_lambda_init", 0.0))
    I.stop_after_polls = int(case.get("stop_after_polls", 0))
    byte = np.uint8(fill)
    def filled(shape, dt):
        shape = tuple(max(int(v), 0) for v in shape)   # a negative count is the library's to refuse
        return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, byte, np.uint8).view(dt).reshape(shape)
    o = dict(cam_q=filled((nf, 4), np.float32), cam_t=filled((nf, 3), np.float32), point=filled((n_points, 3), np.float32),
             chi2=filled((n_edges,), np.float64), flags=filled((n_edges,), np.uint8), q=filled((nf, 4), np.float64),
             t=filled((nf, 3), np.float64), X=filled((n_points, 3), np.float64))
    O = L.LbaOutput()
    C.memset(C.byref(O), int(byte), C.sizeof(O))
    O.cam_q, O.cam_t, O.point, O.chi2, O.flags = [L.ptr(o[k]) for k in ("cam_q", "cam_t", "point", "chi2", "flags")]
    O.diag.cam_q, O.diag.cam_t, O.diag.point = L.ptr(o["q"]), L.ptr(o["t"]), L.ptr(o["X"])

    def call(_keep=(a, pool)):
        if handle is None:
            L.check(lib, lib.rgbl_local_bundle_adjustment_host(C.byref(I), C.byref(O)))
        else:
            L.check(lib, lib.rgbl_local_bundle_adjustment(handle, C.byref(I), C.byref(O)))
        r = dict(o)
        for k, _ in L.LbaDiag._fields_[:11]:
            r[k] = getattr(O.diag, k)
        return r
    call.outputs, call.raw = o, O
    return call


def local_bundle_adjustment_host(case, lib=None, fill=0):
    """rgbl_local_bundle_adjustment_host: the host build of csrc/lba_math.h (no device)."""
    return local_bundle_adjustment_call(lib or L.load(), None, case, fill)()


def bundle_adjustment_call(lib, handle, case, fill=0):
    """The call of rgbl_bundle_adjustment (handle None: rgbl_bundle_adjustment_host) on a case dict: n_cams, cam_is_fixed
    (optional), cam_q, cam_t, cam_K, cam_bf, world_pos (or pool = MapPointPool with slot), edge_point, edge_cam, edge_obs,
    edge_inv_sigma2; optional robust (1), max_iterations (10), stop, stop_byte and stop_after_polls (0).  Every output array
    starts as `fill` bytes.  Returns a callable that gives dict(cam_q, cam_t, point, included, chi2, q, t, X (the estimates in
    double) and the diag's scalars); its .outputs holds the raw arrays."""
    def arr(key, dt):
        v = case.get(key)
        return None if v is None else np.ascontiguousarray(v, dt)
    nc = int(case["n_cams"])
    a = dict(cam_is_fixed=arr("cam_is_fixed", np.uint8), cam_q=arr("cam_q", np.float32), cam_t=arr("cam_t", np.float32),
             cam_K=arr("cam_K", np.float32), cam_bf=arr("cam_bf", np.float32), world_pos=arr("world_pos", np.float32),
             slot=arr("slot", np.int32), edge_point=arr("edge_point", np.int32), edge_cam=arr("edge_cam", np.int32),
             edge_obs=arr("edge_obs", np.float32), edge_inv_sigma2=arr("edge_inv_sigma2", np.float32),
             stop=arr("stop", np.int32), stop_byte=arr("stop_byte", np.uint8))
    pool = case.get("pool")
    n_points = int(case["n_points"]) if "n_points" in case else (len(a["slot"]) if pool is not None else a["world_pos"].size // 3)
    n_edges = int(case["n_edges"]) if "n_edges" in case else (0 if a["edge_point"] is None else len(a["edge_point"]))
    I = L.BaInput()
    I.n_cams, I.n_points, I.n_edges = nc, n_points, n_edges
    for k in ("cam_is_fixed", "cam_q", "cam_t", "cam_K", "cam_bf", "slot", "edge_point", "edge_cam", "edge_obs",
              "edge_inv_sigma2", "stop", "stop_byte"):
        setattr(I, k, L.ptr(a[k]))
    I.world_pos = L.ptr(a["world_pos"]) if pool is None else None
    I.pool = pool.h if pool is not None else None
    I.robust = int(case.get("robust", 1))
    I.max_iterations = int(case.get("max_iterations", 10))
    I.stop_after_polls = int(case.get("stop_after_polls", 0))
    byte = np.uint8(fill)
    def filled(shape, dt):
        shape = tuple(max(int(v), 0) for v in shape)   # a negative count is the library's to refuse
        return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, byte, np.uint8).view(dt).reshape(shape)
    o = dict(cam_q=filled((nc, 4), np.float32), cam_t=filled((nc, 3), np.float32), point=filled((n_points, 3), np.float32),
             included=filled((n_points,), np.uint8), chi2=filled((n_edges,), np.float64), q=filled((nc, 4), np.float64),
             t=filled((nc, 3), np.float64), X=filled((n_points, 3), np.float64))
    O = L.BaOutput()
    C.memset(C.byref(O), int(byte), C.sizeof(O))
    O.cam_q, O.cam_t, O.point, O.included, O.chi2 = [L.ptr(o[k]) for k in ("cam_q", "cam_t", "point", "included", "chi2")]
    O.diag.cam_q, O.diag.cam_t, O.diag.point = L.ptr(o["q"]), L.ptr(o["t"]), L.ptr(o["X"])

    def call(_keep=(a, pool)):
        if handle is None:
            L.check(lib, lib.rgbl_bundle_adjustment_host(C.byref(I), C.byref(O)))
        else:
            L.check(lib, lib.rgbl_bundle_adjustment(handle, C.byref(I), C.byref(O)))
        r = dict(o)
        for k, _ in L.LbaDiag._fields_[:11]:
            r[k] = getattr(O.diag, k)
        return r
    call.outputs, call.raw = o, O
    return call


def bundle_adjustment_host(case, lib=None, fill=0):
    """rgbl_bundle_adjustment_host: the host build of csrc/lba_math.h with lm_solve_panel (no device)."""
    return bundle_adjustment_call(lib or L.load(), None, case, fill)()


def two_view_reconstruct_host(problem, lib=None, diag=True, fill=0):
    """rgbl_two_view_reconstruct_host: TwoViewReconstruction by the host build of csrc/twoview_math.h (no device, no handle); the
    result dict of ORBmatcher.TwoViewReconstruct."""
    lib = lib or L.load()
    keep = []
    I, O = ORBmatcher._two_view_input(problem, keep), L.TwoViewOutput()
    bufs = ORBmatcher._two_view_buffers(I, O, fill, diag)
    L.check(lib, lib.rgbl_two_view_reconstruct_host(C.byref(I), C.byref(O)))
    return ORBmatcher._two_view_result(O, bufs)
