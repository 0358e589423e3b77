#!/usr/bin/env python3
"""The stride-2 data gradient of the first discriminator block's down-sampling layer in isolation (hg_conv2d_dgrad, 16 -> 16
channels, 256 x 256 gradient map, batch 64: 67 MB of gout in, 268 MB of gin out) for rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
passes (tools/s2_dgrad_traffic.sh)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from histogan_amd import conv as C
dev = torch.device('cuda:0')
B, Ch, S = 64, 16, 256
w = torch.randn(Ch, Ch, 3, 3, device=dev) / (Ch * 9) ** 0.5
go = torch.randn(B, Ch, S // 2, S // 2, device=dev)
wd = C.pack_weights(w, C.PACK_DGRAD)
for _ in range(int(os.environ.get('HG_ONE_ITERS', 4))):
    C.conv_dgrad_packed(go, wd, Ch, S, S, 3, 2)
torch.cuda.synchronize()
