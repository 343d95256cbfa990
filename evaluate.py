"""Command-line entry of the held-out log-likelihood evaluation, beside generate.py and fid.py: `python3 evaluate.py --config
codes/<exp>_config.json --n-samples 5000` (implementation and options: ladder_latent_data_distribution_modelling_amd/evaluate.py; also
`python -m ladder_latent_data_distribution_modelling_amd.evaluate`)."""
from ladder_latent_data_distribution_modelling_amd.evaluate import main

if __name__ == "__main__":
    main()
