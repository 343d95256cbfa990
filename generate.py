"""Command-line entry of bulk generation, beside train.py: `python3 generate.py --config codes/<exp>_config.json --n N --out F.npz`
(implementation and options: ladder_latent_data_distribution_modelling_amd/generate.py; also `python -m
ladder_latent_data_distribution_modelling_amd.generate`)."""
from ladder_latent_data_distribution_modelling_amd.generate import main

if __name__ == "__main__":
    main()
