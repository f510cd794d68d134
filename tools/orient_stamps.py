"""Phase breakdown of k_orient_brief from a library built with -DRGBL_ORIENT_STAMPS (make HIPFLAGS+=... ; never the shipped
build): python tools/orient_stamps.py [W H NFEATURES BATCH].  Prints the mean device-clock ticks per wave and phase."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from orb_slam3_rgbl_amd import _lib as L, frontend as F, synth
lib = L.load()
W, H, NF, B = (int(v) for v in (sys.argv[1:5] if len(sys.argv) > 4 else (1241, 376, 2000, 64)))
ex = F.ORBextractor(NF, 1.2, 8, 12, 7, W, H, max_batch=B, lib=lib)
s = synth.Sequence(0, W, H, n_frames=B, constant_density=True)
imgs = np.stack([s.frame(i) for i in range(B)])


def read():
    st = np.zeros(16, np.uint64)
    L.check(lib, lib.rgbl_extractor_debug_stamps(ex.h, st.ctypes.data, len(st)))
    return st.astype(np.int64)


ex.extract_batch(imgs)   # warm-up
a = read()
ex.extract_batch(imgs)
d = read() - a
if d[7] == 0:
    raise SystemExit("no stamps: the library was not built with -DRGBL_ORIENT_STAMPS")
d[2] -= d[1]
names = ("setup + requests issued", "wait for + moments of the first raw patch", "other moments", "barriers + angle / sin / cos",
         "pass 2 (steered BRIEF)", "keypoint record")
tot = float(d[:6].sum())
print("k_orient_brief, %d x %dx%d frames: %d waves with keypoints, %.0f ticks per wave" % (B, W, H, d[7], tot / d[7]))
for n, v in zip(names, d[:6]):
    print("  %-44s %8.0f ticks  %5.1f %%" % (n, v / d[7], 100.0 * v / tot))
