"""k-means / DP-means clustering of CPC features and quantization into discrete units (the reference's cpc/clustering) on
the MI355X kernels of csrc/kmeans.hip."""
