"""The file layout of the DeepLabV3 golden fixtures (tests/golden/g19_deeplab_<H>x<W>.npz), shared by
devtools/gen_deeplab_goldens.py, which writes them, and by the tests, which read them.  A fixture is one .npz with the fields
of the PSPNet ones.  No committed file may exceed 1 MiB, and float32 logits do not compress: where the single file would be
larger (153 x 153: 21 x 153 x 153 logits alone are 1.97 MB), the logits leave it and go, split along the class axis, into
sibling files g19_deeplab_<H>x<W>.logits<k>.npz (field ``logits``: classes [k * LOGIT_CLASSES_PER_PART, ...)); the main
file then holds ``logit_parts``, their number.  ``load`` returns the same dictionary either way."""
import os

import numpy as np

MAX_BYTES = 1 << 20
LOGIT_CLASSES_PER_PART = 7


def path(golden_dir, H, W):
    return os.path.join(golden_dir, f"g19_deeplab_{H}x{W}.npz")


def part_path(golden_dir, H, W, k):
    return os.path.join(golden_dir, f"g19_deeplab_{H}x{W}.logits{k}.npz")


def save(golden_dir, H, W, fields):
    """write the fixture; returns the list of files written"""
    main = path(golden_dir, H, W)
    np.savez_compressed(main, **fields)
    if os.path.getsize(main) <= MAX_BYTES:
        return [main]
    logits = fields["logits"]
    chunks = [logits[:, c:c + LOGIT_CLASSES_PER_PART] for c in range(0, logits.shape[1], LOGIT_CLASSES_PER_PART)]
    rest = {k: v for k, v in fields.items() if k != "logits"}
    np.savez_compressed(main, logit_parts=np.int64(len(chunks)), **rest)
    files = [main]
    for k, chunk in enumerate(chunks):
        np.savez_compressed(part_path(golden_dir, H, W, k), logits=np.ascontiguousarray(chunk))
        files.append(part_path(golden_dir, H, W, k))
    return files


def files(golden_dir, H, W):
    main = path(golden_dir, H, W)
    with np.load(main) as g:
        n = int(g["logit_parts"]) if "logit_parts" in g.files else 0
    return [main] + [part_path(golden_dir, H, W, k) for k in range(n)]


def load(golden_dir, H, W):
    """the fixture as a dictionary of numpy arrays, ``logits`` re-assembled"""
    with np.load(path(golden_dir, H, W)) as g:
        out = {k: g[k] for k in g.files}
    n = out.pop("logit_parts", None)
    if n is not None:
        parts = []
        for k in range(int(n)):
            with np.load(part_path(golden_dir, H, W, k)) as p:
                parts.append(p["logits"])
        out["logits"] = np.concatenate(parts, axis=1)
    return out
