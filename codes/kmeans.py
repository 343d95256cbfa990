"""Alias of ladder_latent_data_distribution_modelling_amd/codes/kmeans.py (device-resident k-means: the labels of a cold mixture fit)."""
from ladder_latent_data_distribution_modelling_amd.codes.kmeans import *  # noqa: F401,F403
from ladder_latent_data_distribution_modelling_amd.codes.kmeans import DeviceKMeans  # noqa: F401
