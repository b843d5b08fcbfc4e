"""Look at a displaced surface: pinhole primary rays through gfx_tfdm_trace, the normals and the depth written as images.

    python tools/tfdm_view.py [--mesh quad|bunny|teapot] [--height FILE] [--size 256] [--scale 0.05] [--level 0] [--box]
                              [--tex-scale 1] [--rotation 0] [--width 960] [--height-px 540] [--out tfdm_view]

--height: a .png / .jpg / .tga / .dds height map (gfxh_tfdm_load_height); without it a procedural map of --size.  --scale is
relative to the mesh's extent.  Writes <out>_normal.png (n * 0.5 + 0.5 in object space) and <out>_depth.png (near = bright), and
prints the hit share and the traversal counters per ray."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gfxexp_amd import api  # noqa: E402
import tfdm_common as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="quad", choices=["quad", "bunny", "teapot"])
    ap.add_argument("--height")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--box", action="store_true")
    ap.add_argument("--tex-scale", type=float, default=1.0)
    ap.add_argument("--rotation", type=float, default=0.0)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height-px", type=int, default=540)
    ap.add_argument("--out", default="tfdm_view")
    a = ap.parse_args()
    heights = api.tfdm_load_height(a.height) if a.height else K.procedural_map(a.size)
    v, t, pos, target, up = K.base_mesh(a.mesh)
    gp = api.tfdm_params(h_scale=a.scale * K.extent(v), tex_scale=(a.tex_scale, a.tex_scale), tex_rotation=a.rotation, target_mip_level=a.level,
                         local_intersection=api.TFDM_BOX if a.box else api.TFDM_TWO_TRIANGLE)
    ctx = api.Context(0)
    tf = api.Tfdm(ctx, v, t, heights, gp)
    w, h = a.width, a.height_px
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target, up=up), w, h)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(w * h * 8, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    tf.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), w * h, d_out.data_ptr(), d_cnt.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hits = d_out.cpu().numpy().view(api.TFDM_HIT_DTYPE)
    cnt = d_cnt.cpu().numpy()
    hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    img = np.zeros((w * h, 4), np.float32)
    img[:, 3] = 1
    img[hit, :3] = hits["normal"][hit] * 0.5 + 0.5
    sdr = api.sdr_config(brightness=1.0, tone_map=False, gamma=False)
    api.save_image_sdr(a.out + "_normal.png", img, w, h, sdr)
    depth = np.zeros((w * h, 4), np.float32)
    depth[:, 3] = 1
    if hit.any():
        d = hits["dist"][hit]
        depth[hit, :3] = (1.0 - 0.9 * (d - d.min()) / max(float(d.max() - d.min()), 1e-30))[:, None]
    api.save_image_sdr(a.out + "_depth.png", depth, w, h, sdr)
    print(json.dumps({"mesh": a.mesh, "size": int(heights.shape[0]), "triangles": int(len(t)), "rays": w * h, "hit_share": round(float(hit.mean()), 4),
                      "aabb_tests_per_ray": round(float(cnt[0]) / (w * h), 2), "leaf_tests_per_ray": round(float(cnt[1]) / (w * h), 2),
                      "base_triangles_per_ray": round(float(cnt[3]) / (w * h), 2), "device_bytes": tf.device_bytes(),
                      "images": [a.out + "_normal.png", a.out + "_depth.png"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
