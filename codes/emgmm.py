"""Alias of ladder_latent_data_distribution_modelling_amd/codes/emgmm.py (device-resident EM GMM fit of the "GMM" prior)."""
from ladder_latent_data_distribution_modelling_amd.codes.emgmm import *  # noqa: F401,F403
from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture  # noqa: F401
