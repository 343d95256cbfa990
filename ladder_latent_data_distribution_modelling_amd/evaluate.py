"""Held-out log-likelihood of a trained model: the importance-weighted estimate log p(x) ~ log (1/S) sum_s w_s (log_likelihood.py), the number
the VampPrior, hierarchical-VAE and GMM-prior baselines are compared by.

    python3 evaluate.py --config codes/mnist_fashion_config.json --n-samples 5000 [--images test.npz] [--max-images N] [--rows R] [--sigma S]
                        [--gm PATH] [--seed S] [--batch-size B] [--out F.npz]

The checkpoints are restored through `model.load` from the directories the config names (as generate.py does); the mixture of the priors "ours" /
"GMM" is read from <result_dir>GM_prior_info.npz or --gm (keys w_full / m_full / K_full, the accurate fit).  Images: the first array of --images
([N, H, W, C]; uint8 is scaled by 1/255), else the config's test split (MNIST: the 10 000 test images, CelebA: celebA_test.tfrecords; seeded synthetic
images when the data files are absent).  --sigma fixes the scale of the pixel likelihood; by default it is |sigma/Variable| of the restored model.
Prints ONE JSON line: mean_log_px, stderr_log_px, mean_elbo_1, mean_ess, n_images, n_samples, sigma, prior.
"""
import argparse
import json
import os
import sys

PRIORS_WITH_OWN_CHECKPOINT = ("ours", "hierarchical", "vampPrior")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="evaluate.py", description="Importance-weighted test log-likelihood of a trained LaDDer model (MI355X HIP path)")
    ap.add_argument("-c", "--config", metavar="C", required=True, help="the configuration file the model was trained with")
    ap.add_argument("--n-samples", type=int, default=5000, help="importance samples per image (the VampPrior paper: 5000)")
    ap.add_argument("--images", metavar="F.npz", default=None, help="archive whose first array holds the images [N, H, W, C] (default: the test split)")
    ap.add_argument("--max-images", type=int, default=None, help="evaluate only the first N images")
    ap.add_argument("--rows", type=int, default=128, help="decoder rows per chunk: max(1, rows // batch) samples of every image at a time")
    ap.add_argument("--sigma", type=float, default=None, help="scale of the pixel likelihood (default: |sigma/Variable| of the model)")
    ap.add_argument("--gm", metavar="PATH", default=None, help="mixture archive (default: <result_dir>GM_prior_info.npz)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the estimator's own Philox stream")
    ap.add_argument("--batch-size", type=int, default=None, help="images encoded together (default: the config's batch_size)")
    ap.add_argument("--out", metavar="F.npz", default=None, help="also write the per-image arrays log_px, elbo_1, ess")
    a = ap.parse_args(argv)
    if a.n_samples < 1 or a.rows < 1 or (a.max_images is not None and a.max_images < 1) or (a.batch_size is not None and a.batch_size < 1):
        ap.error("--n-samples, --rows, --max-images and --batch-size must be >= 1")
    if a.sigma is not None and not a.sigma > 0:
        ap.error("--sigma must be > 0")
    return a


def load_images(path, cfg, max_images):
    import numpy as np
    if path is not None:
        if not os.path.isfile(path):
            sys.exit("evaluate.py: no image archive at %s" % path)
        d = np.load(path)
        x = d[d.files[0]] if hasattr(d, "files") else d
        if x.ndim == 3:
            x = x[..., None]
        x = x[:max_images]
        return x.astype(np.float32) * np.float32(1.0 / 255) if x.dtype == np.uint8 else np.asarray(x, np.float32)
    from .codes.data_loader import DataGenerator
    data = DataGenerator(cfg, None)
    if cfg["exp_name"] == "celeba":
        return data.celeba_images("test", limit=max_images)
    return data.val_set["image"][:max_images]


def run(config_file, n_samples=5000, images=None, max_images=None, rows=128, sigma=None, gm=None, seed=0, batch_size=None):
    import numpy as np
    from .codes import models, utils
    from .codes.session import Session
    from .log_likelihood import FULL_MIXTURE_PRIORS, ImportanceEstimator
    cfg = utils.process_config(config_file)
    model_cls = {"mnist_digit": models.MNISTModel_digit, "mnist_fashion": models.MNISTModel_fashion, "celeba": models.CelebAModel_densenet}[cfg["exp_name"]]
    mixture = None
    if cfg["prior"] in FULL_MIXTURE_PRIORS:
        path = gm or "{}GM_prior_info.npz".format(cfg["result_dir"])
        if not os.path.isfile(path):
            sys.exit("evaluate.py: no fitted mixture at %s (train to an accurate fit first, or pass --gm)" % path)
        g = np.load(path)
        mixture = (g["w_full"], g["m_full"], g["K_full"])
    x = load_images(images, cfg, max_images)
    shape = (int(cfg["dim_input_x"]), int(cfg["dim_input_y"]), int(cfg["dim_input_channel"]))
    if x.ndim != 4 or tuple(x.shape[1:]) != shape or x.shape[0] < 1:
        sys.exit("evaluate.py: images of shape %s do not fit the model's %s" % (tuple(x.shape), ("N",) + shape))
    model = model_cls(cfg)
    session = Session(model)
    for which in ("VAE",) + (("prior",) if cfg["prior"] in PRIORS_WITH_OWN_CHECKPOINT else ()):
        model.load(session, model=which)
    est = ImportanceEstimator(model.engine, mixture, sigma=sigma, seed=seed)
    res = est.estimate(x, n_samples=n_samples, rows=rows, batch_size=batch_size)
    res["prior"] = cfg["prior"]
    return res


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    res = run(a.config, a.n_samples, a.images, a.max_images, a.rows, a.sigma, a.gm, a.seed, a.batch_size)
    if a.out:
        np.savez(a.out, **{k: v for k, v in res.items() if k != "prior"})
    print(json.dumps({k: res[k] for k in ("mean_log_px", "stderr_log_px", "mean_elbo_1", "mean_ess", "n_images", "n_samples", "sigma", "prior")}))


if __name__ == "__main__":
    main()
