#!/usr/bin/env python3
"""A/B of two builds of the library on the gradients of a fixed step: run once per build, then diff the dumps.
    AVA_HIP_LIB_TAG=prev python tools/ab_grads.py dump /tmp/a.npz ; python tools/ab_grads.py dump /tmp/b.npz ; python tools/ab_grads.py diff /tmp/a.npz /tmp/b.npz
The step of a dump is chosen by environment variables: AB_B (batch, 8), AB_Z (latent size, 64), AB_SHAPE (HxW, 128x128),
AB_ACT (float32 | bfloat16), AB_EVAL=1 (the forward runs in eval mode), AB_SCALE (backward of loss * AB_SCALE),
AB_PARTS=1 (the backward runs as ava_backward_part 0 .. 3 instead of ava_backward)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def dump(out, B=8, z=64, shape=(128, 128), act="float32", eval_mode=False, scale=1.0, parts=False):
    """One forward + backward of the fixture model on the fixture batch; loss and the 80 gradient tensors to `out` (.npz)."""
    import torch
    from ava_amd import _lib, synthetic as syn, layout
    from ava_amd.vae import VAE
    model = VAE(z_dim=z, device_name="cuda", x_shape=shape, act_dtype=act)
    fp = syn.fixture_parameters(z, shape)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            prm.copy_(torch.from_numpy(fp[name]))
    model.train(not eval_mode)
    ew, ed = syn.noise(B, z)
    model.noise_source = lambda b, zz: (ew, ed)
    x = torch.from_numpy(syn.spectrograms(B, shape=shape)).cuda()
    model.optimizer.zero_grad()
    loss = model.forward(x)
    if parts:
        lib = _lib.load()
        for part in range(lib.ava_backward_num_parts()):
            _lib.check(lib.ava_backward_part(model._handle, x.data_ptr(), B, part, _lib.stream()), "ava_backward_part")
    else:
        (loss * scale if scale != 1.0 else loss).backward()
    torch.cuda.synchronize()
    offs, total = layout.arena_offsets(z, x_shape=shape)
    g = model._grads.cpu().numpy()
    np.savez(out, loss=float(loss.item()), **{s.name: g[offs[s.name]:offs[s.name] + s.numel] for s in layout.param_specs(z, shape)})


def diff(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    print("loss", float(a["loss"]), float(b["loss"]))
    worst = []
    for k in a.files:
        if k == "loss":
            continue
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()
        n = np.abs(a[k]).max() + 1e-30
        worst.append((d / n, k))
    print("%d tensors, %d differ, worst max|diff|/max|a| = %.3e" % (len(worst), sum(r != 0 for r, _ in worst), max(worst)[0]))
    for r, k in sorted(worst)[::-1][:20]:
        print("%-18s max|diff|/max|a| = %.3e" % (k, r))


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        env = os.environ.get
        dump(sys.argv[2], int(env("AB_B", "8")), int(env("AB_Z", "64")), tuple(int(v) for v in env("AB_SHAPE", "128x128").split("x")),
             env("AB_ACT", "float32"), env("AB_EVAL", "0") == "1", float(env("AB_SCALE", "1")), env("AB_PARTS", "0") == "1")
    else:
        diff(sys.argv[2], sys.argv[3])
