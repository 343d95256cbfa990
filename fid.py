"""Command-line entry of the FID evaluation, beside generate.py: `python3 fid.py --real a.npz --generated b.npz --weights vgg16.npz`
(implementation and options: ladder_latent_data_distribution_modelling_amd/fid.py; also `python -m
ladder_latent_data_distribution_modelling_amd.fid`)."""
from ladder_latent_data_distribution_modelling_amd.fid import main

if __name__ == "__main__":
    main()
