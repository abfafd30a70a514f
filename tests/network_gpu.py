"""The network through its raw C entry (uoc_net_create_mode .. uoc_net_forward), for the tests that hold the embeddings to
the fp64 reference, and the child process of the tuner test (test infrastructure, never product code).

As a program it computes the RGBD_ADD embeddings of the tuner test's two shapes under whatever UOC_CONV_* environment its
parent set and saves them as .npy (the tuner reads its environment once per process, so every variant is a fresh process):

    python tests/network_gpu.py <output directory>
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unseenobjectclustering_amd import _native  # noqa: E402

MODE_ID = {"RGBD_ADD": 0, "COLOR": 1, "DEPTH": 2, "RGBD_EARLY": 3, "RGBD_CAT": 4}     # include/uoc_hip.h UOC_NET_*
TUNER_SHAPES = ((37, 53, (31, 32)), (224, 224, (51, 52)))                              # (H, W, frame seeds): B = 2 each


class RawNet:
    """A native network built from a state dict of numpy arrays or tensors."""

    def __init__(self, device, sd, mode):
        self.device, self.mode, self.handle = device, mode, None
        h = ctypes.c_void_p()
        _native.call("uoc_net_create_mode", None, ctypes.byref(h), MODE_ID[mode])
        self.handle = h
        for key, v in sd.items():
            if key.endswith("num_batches_tracked"):
                continue
            t = torch.as_tensor(np.asarray(v)).to(torch.float32).contiguous()
            _native.check(_native.lib().uoc_net_load_param(h, key.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()),
                          f"uoc_net_load_param({key})")
        _native.call("uoc_net_finalize", device, h, stream=False)

    def set_split_precision(self, on):
        _native.call("uoc_net_set_split_precision", self.device, self.handle, 1 if on else 0, stream=False)

    def forward(self, img, depth):
        """img, depth [B,3,H,W] float32 on the CPU (the mode's unused one is not passed) -> the embeddings on the device as
        the kernels write them, [B,H*W,64] or for RGBD_CAT [B,2,H*W,64].  The output is filled with NaN before the call: a
        pixel the network does not write cannot pass."""
        B, _, H, W = img.shape
        cat = self.mode == "RGBD_CAT"
        a = img.contiguous().to(self.device) if self.mode != "DEPTH" else None
        d = depth.contiguous().to(self.device) if self.mode != "COLOR" else None
        embed = torch.full((B, 2, H * W, 64) if cat else (B, H * W, 64), float("nan"), device=self.device)
        nbytes = _native.lib().uoc_net_workspace_bytes(self.handle, B, H, W)
        assert nbytes > 0, (B, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert ws.data_ptr() % 256 == 0
        _native.call("uoc_net_forward", self.device, self.handle, a, d, B, H, W, embed, ws, ws.numel())
        torch.cuda.synchronize(self.device)
        return embed

    def close(self):
        if self.handle is not None:
            _native.lib().uoc_net_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nchw(embed, H, W):
    """The kernels' layout -> [B,64|128,H,W] on the CPU."""
    e = embed.cpu()
    if e.dim() == 4:
        B = e.shape[0]
        return e.view(B, 2, H, W, 64).permute(0, 1, 4, 2, 3).reshape(B, 128, H, W)
    return e.view(e.shape[0], H, W, 64).permute(0, 3, 1, 2)


def main(out_dir):
    from tests import network_reference as NR
    assert torch.cuda.is_available(), "needs a GPU"
    device = torch.device("cuda:0")
    net = RawNet(device, NR.state_dict("RGBD_ADD"), "RGBD_ADD")
    for H, W, seeds in TUNER_SHAPES:
        img, depth = NR.frames(seeds, H, W)
        e = net.forward(img, depth).cpu().numpy()
        assert np.isfinite(e).all()
        np.save(os.path.join(out_dir, f"embed_{H}x{W}.npy"), e)
    net.close()


if __name__ == "__main__":
    main(sys.argv[1])
