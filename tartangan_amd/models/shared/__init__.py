"""The shared-filter model family (reference models/shared): one 3x3 filter bank per network, bilinear resampling."""
