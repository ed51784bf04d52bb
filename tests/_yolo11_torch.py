"""TEST INFRASTRUCTURE -- an independent torch fp32 restatement of YOLO11 (detect and pose), module by module.

Written from the Ultralytics module definitions (nn/modules/block.py: C3k2, C3k, Bottleneck, C2PSA, PSABlock, Attention, SPPF;
nn/modules/conv.py: Conv, DWConv; nn/modules/head.py: Detect with legacy=False, Pose) and yolo11.yaml, in their own operation
order: ``F.conv2d(groups=c)``, ``(q.transpose(-2, -1) @ k) * scale``, ``.softmax(-1)``, ``v @ attn.transpose(-2, -1)``.  It does
NOT use the product's program builder (cvsd_amd.graph): it exists to catch graph-building mistakes (channel splits, row
permutations, residual placement) that a float64 run of the product's own program would share.  The BN fold, the Detect decode
and the SPPF / Upsample / Concat plumbing come from oracle/yolo_oracle.py.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.yolo_oracle import OracleModel

# yolo11.yaml scales: (depth, width, max_channels)
SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}
# yolo11.yaml backbone + head: (from, repeats, module, args)
YAML = [
    (-1, 1, "Conv", [64, 3, 2]), (-1, 1, "Conv", [128, 3, 2]), (-1, 2, "C3k2", [256, False, 0.25]),
    (-1, 1, "Conv", [256, 3, 2]), (-1, 2, "C3k2", [512, False, 0.25]), (-1, 1, "Conv", [512, 3, 2]),
    (-1, 2, "C3k2", [512, True]), (-1, 1, "Conv", [1024, 3, 2]), (-1, 2, "C3k2", [1024, True]),
    (-1, 1, "SPPF", [1024, 5]), (-1, 2, "C2PSA", [1024]),
    (-1, 1, "Upsample", []), ([-1, 6], 1, "Concat", []), (-1, 2, "C3k2", [512, False]),
    (-1, 1, "Upsample", []), ([-1, 4], 1, "Concat", []), (-1, 2, "C3k2", [256, False]),
    (-1, 1, "Conv", [256, 3, 2]), ([-1, 13], 1, "Concat", []), (-1, 2, "C3k2", [512, False]),
    (-1, 1, "Conv", [512, 3, 2]), ([-1, 10], 1, "Concat", []), (-1, 2, "C3k2", [1024, True]),
    ([16, 19, 22], 1, "Head", []),
]


class Yolo11Torch(OracleModel):
    def __init__(self, name: str, state_dict: Dict[str, np.ndarray], nc: Optional[int] = None):
        n = name.lower().replace("-pose", "")
        assert n.startswith("yolo11") and len(n) == 7, name
        self.scale = n[6]
        self.half = False
        self.yaml = YAML
        self.depth, self.width, self.max_ch = SCALES[self.scale]
        self.pose = name.lower().endswith("-pose")
        self.nc = nc if nc is not None else (1 if self.pose else 80)
        self.kpt_shape = (17, 3) if self.pose else (0, 0)
        self.nk = self.kpt_shape[0] * self.kpt_shape[1]
        self.reg_max = 16
        self.sd = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).clone() for k, v in state_dict.items()}
        self._fused = {}
        self.stride = [8, 16, 32]

    # nn/modules/conv.py:Conv.forward_fuse with act=True (SiLU) or act=False (Identity); DWConv = Conv(g=c1)
    def Cv(self, x, prefix, k=1, s=1, act=True, g=1):
        w, b = self._fused_conv(prefix)
        y = F.conv2d(x, w, b, stride=s, padding=k // 2, groups=g)
        return F.silu(y) if act else y

    # block.py:Bottleneck(c1, c2, shortcut, g, k, e): add = shortcut and c1 == c2
    def Bneck(self, x, prefix, shortcut=True):
        y = self.Cv(self.Cv(x, prefix + ".cv1", 3), prefix + ".cv2", 3)
        return x + y if shortcut and y.shape[1] == x.shape[1] else y

    # block.py:C3k(c1, c2, n=2, shortcut, g, e=0.5, k=3): C3 with Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0)
    def C3k(self, x, prefix, n=2, shortcut=True):
        a = self.Cv(x, prefix + ".cv1")
        for i in range(n):
            a = self.Bneck(a, f"{prefix}.m.{i}", shortcut)
        return self.Cv(torch.cat((a, self.Cv(x, prefix + ".cv2")), 1), prefix + ".cv3")

    # block.py:C3k2 (a C2f): y = list(cv1(x).chunk(2, 1)); y.extend(m(y[-1]) for m in self.m); cv2(cat(y))
    def C3k2(self, x, prefix, n, c3k, shortcut=True):
        y = list(self.Cv(x, prefix + ".cv1").chunk(2, 1))
        for i in range(n):
            y.append(self.C3k(y[-1], f"{prefix}.m.{i}", 2, shortcut) if c3k else self.Bneck(y[-1], f"{prefix}.m.{i}", shortcut))
        return self.Cv(torch.cat(y, 1), prefix + ".cv2")

    # block.py:Attention(dim, num_heads, attn_ratio=0.5)
    def Attention(self, x, prefix, num_heads):
        B, C, H, W = x.shape
        N = H * W
        head_dim = C // num_heads
        key_dim = int(head_dim * 0.5)
        scale = key_dim ** -0.5
        qkv = self.Cv(x, prefix + ".qkv", act=False)
        q, k, v = qkv.view(B, num_heads, key_dim * 2 + head_dim, N).split([key_dim, key_dim, head_dim], dim=2)
        attn = (q.transpose(-2, -1) @ k) * scale
        attn = attn.softmax(dim=-1)
        x = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.Cv(v.reshape(B, C, H, W), prefix + ".pe", 3, act=False, g=C)
        return self.Cv(x, prefix + ".proj", act=False)

    # block.py:PSABlock(c, attn_ratio=0.5, num_heads=c // 64, shortcut=True)
    def PSABlock(self, x, prefix):
        c = x.shape[1]
        x = x + self.Attention(x, prefix + ".attn", c // 64)
        return x + self.Cv(self.Cv(x, prefix + ".ffn.0"), prefix + ".ffn.1", act=False)

    # block.py:C2PSA(c1, c2, n, e=0.5)
    def C2PSA(self, x, prefix, n):
        c = int(x.shape[1] * 0.5)
        a, b = self.Cv(x, prefix + ".cv1").split((c, c), dim=1)
        for i in range(n):
            b = self.PSABlock(b, f"{prefix}.m.{i}")
        return self.Cv(torch.cat((a, b), 1), prefix + ".cv2")

    def SPPF5(self, x, prefix):
        y = [self.Cv(x, prefix + ".cv1")]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], kernel_size=5, stride=1, padding=2))
        return self.Cv(torch.cat(y, 1), prefix + ".cv2")

    def _seq3(self, x, prefix):
        """head branches; Detect(legacy=False).cv3[i] = [DWConv(x, x, 3), Conv(x, c3, 1)], [DWConv(c3, c3, 3), Conv(c3, c3, 1)],
        nn.Conv2d(c3, nc, 1); cv2 / cv4 as in v8."""
        if ".cv3." in prefix:
            for j in range(2):
                x = self.Cv(self.Cv(x, f"{prefix}.{j}.0", 3, g=x.shape[1]), f"{prefix}.{j}.1")
        else:
            x = self.Cv(self.Cv(x, prefix + ".0", 3), prefix + ".1", 3)
        return F.conv2d(x, self.sd[prefix + ".2.weight"], self.sd[prefix + ".2.bias"])

    @torch.no_grad()
    def forward(self, x: torch.Tensor, return_features: bool = False):
        ys = []
        for i, (f, n, m, args) in enumerate(self.yaml):
            n = max(round(n * self.depth), 1) if n > 1 else n
            xin = x if i == 0 else (ys[f if f >= 0 else i + f] if isinstance(f, int) else [ys[j if j >= 0 else i + j] for j in f])
            p = f"model.{i}"
            if m == "Conv":
                out = self.Cv(xin, p, args[1], args[2])
            elif m == "C3k2":
                out = self.C3k2(xin, p, n, args[1] or self.scale in "mlx")       # parse_model: c3k forced for m / l / x
            elif m == "C2PSA":
                out = self.C2PSA(xin, p, n)
            elif m == "SPPF":
                out = self.SPPF5(xin, p)
            elif m == "Upsample":
                out = F.interpolate(xin, scale_factor=2.0, mode="nearest")
            elif m == "Concat":
                out = torch.cat(xin, 1)
            else:
                if return_features:
                    return xin
                out = self.Head(xin, p)
            ys.append(out)
        return ys[-1]

    def count_params(self) -> int:
        return sum(v.numel() + (v.shape[0] if k.endswith("conv.weight") and ".dfl." not in k else 0)
                   for k, v in self.sd.items() if k.endswith(("conv.weight", ".2.weight", ".2.bias")) or ".dfl." in k)


def head(name: str, sd, frames: np.ndarray, imgsz: int = 640, nc: Optional[int] = None) -> np.ndarray:
    """[N, no, A] fp32 pre-NMS head tensor of uint8 BGR frames."""
    from oracle import yolo_oracle as O
    return Yolo11Torch(name, sd, nc).forward(O.preprocess(list(frames), imgsz)).numpy()

