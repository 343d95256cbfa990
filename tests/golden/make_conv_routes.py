"""Records tests/golden/conv_routes.json on a GPU: for the three shipped configs at their batch sizes, in f32 and f16x3, the library entry points
that every Conv2D.forward / .backward / .forward_up2 / .forward_fused_proj call of one training iteration + one evaluation launches (the calls
are spied at _lib.call and tagged with the layer and pass they belong to).  tests/test_host_cpu.py::test_conv_routes_match_recorded_launches holds
Conv2D.route to it, so the file is recorded from launches, never from the planner: `python tests/golden/make_conv_routes.py [OUT.json]`."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ladder_latent_data_distribution_modelling_amd import _lib as L  # noqa: E402
from ladder_latent_data_distribution_modelling_amd import layers  # noqa: E402
from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine  # noqa: E402

stack, records = [], []
_call = L.call


def spy(name, *args):
    if stack:
        stack[-1]["calls"].append(name)
    return _call(name, *args)


def wrap(meth):
    orig = getattr(layers.Conv2D, meth)

    def tagged(self, *a, **kw):
        rec = dict(layer=self.name, meth=meth, keep=bool(self.ctx.keep_activations))
        if meth == "backward":
            k, sh = self.kept, list(self.kept.x.shape)
            if k.x_kind == "lowres":
                sh[1], sh[2] = k.factor * sh[1], k.factor * sh[2]
            arg = dict(need_dx=True, wgrad=True, act_done=False, gate_prev=None, lowres_dx=False, lowres_gate=None, proj_grad=None)
            arg.update(zip(("dy", "need_dx", "wgrad", "act_done", "gate_prev", "lowres_dx", "lowres_gate", "proj_grad"), a))
            arg.update(kw)
            rec.update(in_shape=[int(v) for v in sh], x_kind=k.x_kind, form=k.form, need_dx=bool(arg["need_dx"]), wgrad=bool(arg["wgrad"]),
                       gated=bool(arg["gate_prev"]), lowres_dx=bool(arg["lowres_dx"]), proj_grad=arg["proj_grad"] is not None)
        else:
            rec.update(in_shape=[int(v) for v in (a[0] if a else kw["x"]).shape])
        rec["calls"] = []
        stack.append(rec)
        try:
            return orig(self, *a, **kw)
        finally:
            stack.pop()
            if rec not in records:
                records.append(rec)
    setattr(layers.Conv2D, meth, tagged)


def main(out):
    L.call = spy
    for meth in ("forward", "backward", "forward_up2", "forward_fused_proj"):
        wrap(meth)
    fixture = {}
    for name in ("celeba", "mnist_digit", "mnist_fashion"):
        for prec in ("f32", "f16x3"):
            cfg = json.load(open(os.path.join(ROOT, "codes", "%s_config.json" % name)))
            cfg["matmul_precision"] = prec
            x = torch.rand(int(cfg["batch_size"]), int(cfg["dim_input_x"]), int(cfg["dim_input_y"]), int(cfg["dim_input_channel"]),
                           generator=torch.Generator().manual_seed(5)).numpy()
            eng = LadderEngine(cfg, "cuda:0", seed=1, noise_seed=99)
            eng.set_sg_mixture()
            del records[:]
            eng.run_ae(x, 2.5e-4, None, False, False)
            eng.evaluate(x, None, False, False)
            torch.cuda.synchronize()
            fixture["%s/%s" % (name, prec)] = dict(batch_size=int(cfg["batch_size"]), up2=int(eng.ctx.up2), records=list(records))
            del eng
            torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_routes.json"))
