#!/usr/bin/env python3
"""GPU box: VNF_WS_STAMP=<file> VNF_AUTOTUNE=0 VNF_FORCE_CFG=64 python tools/stamp_ws.py -> in-kernel stamps of the
wave-specialised kernel on the layers it fits (see conv_ws.hip launch_stamped).  Needs the library built with
python -m vn_celeb_face_recognition_amd.build --stamps; the default build ignores the variable.

One line per wave and K tile (the first 64): "wave kt t0 t1 t2 t3".  t0: at the tile's join, t1: behind its s_waitcnt,
t2: behind the s_barrier.  t3, loader waves: tile kt + S - 1 issued.  t3, consumer waves: taken at the NEXT tile's entry
(and behind the K loop for the last tile), since the stamps are part of the join that the kernel hands to conv_k_loop;
before the shared K loop it was taken right behind the tile's MFMAs, so it now also holds the loop's branch back and,
software-pipelined, still leaves the tile's second half to the next tile."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vn_celeb_face_recognition_amd.models import InceptionResnetV1
m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype="bf16", max_batch=256).eval()
x = torch.randn((256, 3, 160, 160), generator=torch.Generator().manual_seed(0)).cuda().to(torch.bfloat16)
m(x)
torch.cuda.synchronize()
