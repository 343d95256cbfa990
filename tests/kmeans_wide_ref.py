"""Shared by tests/test_kmeans_wide_cpu.py and tests/test_gpu_kmeans_wide.py: the k-means cases on 80 .. 256 dimensions (csrc/kmeans_wide.hip).  The
data, the numpy restatement with its preconditions, sklearn's fit and the decidability check are those of the narrow k-means (tests/kmeans_ref.py):
the wide kernels differ from the narrow ones in how the sums are cut, not in what they compute."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kmeans_ref import NumpyKMeans, assert_labels_are_decidable, data, sklearn_fit  # noqa: E402,F401

# N, R, K, kind, data seed, random_state of the fit, explicit init (None, or "far": K sample rows with the middle centre set to 100.0)
CASES = [
    (1300, 80, 33, "blobs", 10, 10, None),          # the narrowest width (second panel: 16 of 64 columns), K one past two tiles, ragged slice and scan block
    (1000, 144, 17, "normal", 12, 12, None),        # nine column blocks, partial third panel, K one past a tile, many Lloyd iterations
    (2049, 256, 50, "blobs", 11, 11, None),         # the shipped shape's width and K; the last slice and the last scan block hold one sample
    (600, 256, 64, "normal", 13, 13, None),         # both maxima: the LDS and workspace limits
    (333, 96, 1, "normal", 14, 14, None),           # K = 1
    (1500, 128, 6, "normal", 15, 15, "far"),        # one relocation, explicit init
    (700, 256, 12, "blobs", 16, 16, "far"),         # relocation with R equal to the block size
    (4100, 256, 50, "normal", 17, 17, None),        # 32 row splits at full width
]
N_ITER = [2, 15, 2, 4, 2, 30, 3, 14]                # sklearn's n_iter_ per case (sklearn 1.7.2)
IDS = ["%dx%dx%d%s" % (c[0], c[1], c[2], "-init" if c[6] else "") for c in CASES]

# the mixture-level comparisons: the first samples of tests/emgmm_wide_ref.py cases 1 and 2, and the label counts of their k-means
MIX_CASES = (1, 2)
MIX_COUNTS = {1: (500, 529, 471), 2: (1062, 989)}
