"""TEST INFRASTRUCTURE shared by test_gpu_shopformer.py and test_gpu_shopformer2.py: the C forms from before the outputs struct, which
the Python front no longer calls."""
import numpy as np
import torch

from cvsd_amd import _lib


def old_c_forms_equal_forward(model, x, want, xd, stream):
    """raw calls of the 6- and 7-argument C forms, with and without tokens and recon: the bits of ``model.forward``"""
    L, n = _lib.lib(), len(x)
    for extra in (True, False):
        sc, tk, rc = np.zeros(n, np.float32), np.zeros_like(want["tokens"]), np.zeros_like(want["reconstructed_tokens"])
        assert L.mi355_shopformer_score(model._h, x.ctypes.data, n, sc.ctypes.data, tk.ctypes.data if extra else None,
                                        rc.ctypes.data if extra else None) == 0
        assert np.array_equal(sc, want["normality_score"])
        assert not extra or (np.array_equal(tk, want["tokens"]) and np.array_equal(rc, want["reconstructed_tokens"]))
        scd, tkd, rcd = (torch.zeros(a.shape, device=xd.device) for a in (sc, tk, rc))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            assert L.mi355_shopformer_score_device_async(model._h, xd.data_ptr(), n, scd.data_ptr(), tkd.data_ptr() if extra else None,
                                                         rcd.data_ptr() if extra else None, stream.cuda_stream) == 0
        stream.synchronize()
        assert np.array_equal(scd.cpu().numpy(), want["normality_score"])
        assert not extra or (np.array_equal(tkd.cpu().numpy(), want["tokens"]) and np.array_equal(rcd.cpu().numpy(), want["reconstructed_tokens"]))

