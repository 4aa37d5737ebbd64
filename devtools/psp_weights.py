"""The weight rule of the PSPNet golden fixtures (tests/golden/g16_psp_*.npz), shared by devtools/gen_psp_goldens.py,
which applies it to the reference's model, and by the tests, which apply it to this repository's model.  The 49 M
parameters are too large for a fixture: the fixtures hold inputs and outputs only, and the weights are re-derived."""
import zlib

import torch


def seeded_state_dict(template, base_seed=0):
    """Deterministic weights for a PSPNet state dict (the golden fixtures of tests/golden/g16_psp_*.npz): every float
    entry from its own generator seeded with ``base_seed + crc32(key)``, so the rule does not depend on the order in
    which a model creates its modules.  ``template``: a state dict (only keys, shapes and dtypes are read).
      conv weights: randn * sqrt(2 / fan_in) (x 0.2 on each bottleneck's conv3, so the residual stack stays O(1));
      BatchNorm: weight U(0.5, 1.5), bias N(0, 0.1), running_mean N(0, 0.1), running_var U(0.5, 2);
      classifier biases: N(0, 0.1).  Integer entries (num_batches_tracked) are zero."""
    out = {}
    bn_prefixes = {k[:-len("running_mean")] for k in template if k.endswith("running_mean")}
    for key, t in template.items():
        if not t.is_floating_point():
            out[key] = torch.zeros_like(t, device="cpu")
            continue
        g = torch.Generator().manual_seed(int(base_seed) + zlib.crc32(key.encode()))
        shape = tuple(t.shape)
        prefix, name = key.rsplit(".", 1)[0] + ".", key.rsplit(".", 1)[1]
        if prefix in bn_prefixes:
            if name == "weight":
                v = 0.5 + torch.rand(shape, generator=g)
            elif name == "running_var":
                v = 0.5 + 1.5 * torch.rand(shape, generator=g)
            else:                                             # bias, running_mean
                v = 0.1 * torch.randn(shape, generator=g)
        elif name == "weight" and len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            v = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            if ".conv3." in key and key.startswith("layer"):
                v = v * 0.2
        else:                                                 # classifier bias
            v = 0.1 * torch.randn(shape, generator=g)
        out[key] = v.to(t.dtype)
    return out
