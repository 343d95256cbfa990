"""Bulk generation from a trained model: N prior samples decoded to images, written as the `sampled_images` array the reference's FID
evaluation opens (reference codes/utils.py:134-138; the sampling branches of codes/base.py:1065-1122).

    python3 generate.py --config codes/celeba_config.json --n 50000 --out sampled.npz [--mode accurate-GM] [--method ours]
                        [--gm PATH] [--uint8] [--seed S] [--chunk B]

The checkpoints are restored through `model.load` from the directories the config names (as train.py does); the mixture of the priors
"ours" / "GMM" is read from <result_dir>GM_prior_info.npz (what the accurate fit of training saves) or from --gm, keys w_full / m_full /
K_full: the reference samples the FULL fitted mixture.  That archive is the accurate fit, so --mode accepts "accurate-GM" (the default) and
refuses "crude-GM", whose mixture exists only inside a running trainer.  Default output: float32 raw decoder output (the clip to [0, 1] is left to the
consumer's preprocessing, as in the reference); --uint8 writes rint(255 * clip(x, 0, 1)) bytes, a quarter of the size.
"""
import argparse
import os
import sys

from .arch import PRIOR_METHODS

PRIORS_WITH_OWN_CHECKPOINT = ("ours", "hierarchical", "vampPrior")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="generate.py", description="Generate images from the prior of a trained LaDDer model (MI355X HIP path)")
    ap.add_argument("-c", "--config", metavar="C", required=True, help="the configuration file the model was trained with")
    ap.add_argument("--n", type=int, required=True, help="number of images")
    ap.add_argument("--out", metavar="F.npz", required=True, help="output archive (key: sampled_images)")
    ap.add_argument("--mode", choices=("accurate-GM", "crude-GM"), default="accurate-GM",
                    help="which mixture fit to sample, as in the reference; only the accurate fit is ever written to disk, so crude-GM is refused")
    ap.add_argument("--method", choices=PRIOR_METHODS, default=None, help="prior to sample (default: the config's)")
    ap.add_argument("--gm", metavar="PATH", default=None, help="mixture archive (default: <result_dir>GM_prior_info.npz)")
    ap.add_argument("--uint8", action="store_true", help="write quantised bytes instead of float32")
    ap.add_argument("--seed", type=int, default=0, help="seed of the sampler's own Philox stream")
    ap.add_argument("--chunk", type=int, default=128, help="images per decoder batch")
    a = ap.parse_args(argv)
    if a.n < 0 or a.chunk < 1:
        ap.error("--n must be >= 0 and --chunk >= 1")
    if a.mode == "crude-GM":
        ap.error("--mode crude-GM: the per-epoch fit lives only in a running trainer (generate_images(mode='crude-GM')); "
                 "GM_prior_info.npz holds the accurate fit")
    return a


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    from .codes import models, utils
    from .codes.session import Session
    cfg = utils.process_config(a.config)
    method = a.method or cfg["prior"]
    model_cls = {"mnist_digit": models.MNISTModel_digit, "mnist_fashion": models.MNISTModel_fashion, "celeba": models.CelebAModel_densenet}[cfg["exp_name"]]
    model = model_cls(cfg)
    session = Session(model)
    for which in ("VAE",) + (("prior",) if cfg["prior"] in PRIORS_WITH_OWN_CHECKPOINT else ()):
        model.load(session, model=which)
    mixture = None
    if method in ("ours", "GMM"):
        path = a.gm or "{}GM_prior_info.npz".format(cfg["result_dir"])
        if not os.path.isfile(path):
            sys.exit("generate.py: no fitted mixture at %s (train to an accurate fit first, or pass --gm)" % path)
        gm = np.load(path)
        mixture = (gm["w_full"], gm["m_full"], gm["K_full"])
    eng = model.engine
    sampler = eng.prior_sampler(method, mixture, seed=a.seed)
    images = eng.generate(a.n, sampler, chunk=a.chunk, as_uint8=a.uint8)
    np.savez(a.out, sampled_images=images)
    print("{} images ({}, prior {}, mode {}) written to {}".format(images.shape[0], images.dtype, method, a.mode, a.out))


if __name__ == "__main__":
    main()
