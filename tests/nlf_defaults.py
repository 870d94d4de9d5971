"""What the sigma modes that existed before ``sigma='nlf'`` compute, as digests: a float and 'auto' through frames_to_input, clip_forward,
ClipPipeline and LiveStream on seeded frames.  ``digests()`` uses nothing the noise-level function added, so it runs on the commit before it;
profiles/noise_curve.txt records what it gave there and tests/test_gpu_nlf.py holds this tree to those values.

    python tests/nlf_defaults.py          (prints the digests as JSON; needs the GPU)"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def small_model():
    """the c32-sized non-blind network of tests/test_gpu_sigma.py"""
    import torch
    import bsvd_amd
    from helpers import bsvd_keys
    from seeded import seeded_state
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32), 13)
    m = bsvd_amd.BSVD(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32,
                      pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


def rgb_frames(n, H, W, seed):
    import sigma_model as M
    sig = [5, 12, 20, 30, 8, 25]
    return np.stack([M.noisy_u8(M.scene("mixed", H, W, seed + t), sig[t % len(sig)], seed + 50 + t).transpose(1, 2, 0) for t in range(n)])


def digests(model=None):
    import torch
    from bsvd_amd import frame_io as F
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    model = model or small_model()
    out = {}
    for (H, W), pad in (((64, 96), None), ((38, 54), "reflect")):
        tag = "%dx%d" % (H, W)
        frames = rgb_frames(5, H, W, 7)
        u8 = torch.from_numpy(frames).to("cuda:0")
        net = F.network_size(H, W) if pad else None
        for name, sigma in (("const30", 30 / 255.0), ("auto", "auto")):
            x = F.frames_to_input(u8, sigma, pad_to=net)
            out["%s input %s" % (tag, name)] = _sha(x.cpu().numpy())
            y = F.output_to_frames(model.clip_forward(x), crop_to=(H, W) if pad else None)
            out["%s clip %s" % (tag, name)] = _sha(y.cpu().numpy())
            pipe = ClipPipeline(model, sigma=sigma, depth=2, pad=pad)
            out["%s ClipPipeline %s" % (tag, name)] = _sha(np.concatenate(list(pipe.run(iter([frames, frames[:3]])))))
            live = LiveStream(model, sigma=sigma, depth=2, pad=pad, frame_shape=(H, W))
            got = [r for r in (live.feed(f) for f in frames) if r is not None] + live.flush()
            out["%s LiveStream %s" % (tag, name)] = _sha(np.stack(got))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "golden"))
    print(json.dumps(digests(), indent=1))
