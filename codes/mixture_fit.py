"""Alias of ladder_latent_data_distribution_modelling_amd/codes/mixture_fit.py (what the device mixture fits share)."""
from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import *  # noqa: F401,F403
