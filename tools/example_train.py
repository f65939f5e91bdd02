#!/usr/bin/env python3
"""End-to-end example on the build-owned synthetic scene (GPU box): train -> reference-format checkpoint -> resume -> full-frame
render -> mesh (host extractor, then on the device).  Everything a user of the reference's trainer touches, through the drop-in's public surface.

    python tools/example_train.py [--iters 300] [--rays 1024] [--out gpurun_out/example]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import bench as B
import synth_scene
from endosurf_amd import EndoSurfRenderer
from endosurf_amd.trainer import Trainer, cal_psnr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "gpurun_out", "example"))
    ap.add_argument("--mesh-method", default="tetrahedra", choices=["tetrahedra", "cubes"],
                    help="triangulation of the on-device meshes: marching tetrahedra, or the cube table (a third of the vertices and triangles)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = B.CONFIGS[2]
    renderer = EndoSurfRenderer(B.render_cfg(cfg), dict(B.NET_CFG), device=dev)
    trainer = Trainer(renderer, n_iter=args.iters, warm_up_end=max(args.iters // 10, 1))
    sched = synth_scene.schedule(5, args.iters, args.rays)
    ev = {k: torch.from_numpy(v).to(dev) for k, v in synth_scene.eval_batch().items()}
    half = args.iters // 2
    t0 = time.perf_counter()
    for it in range(1, half + 1):
        b = {k: torch.from_numpy(v).to(dev) for k, v in sched[it - 1].items()}
        trainer.update_learning_rate(it)
        loss, terms, _ = trainer.train_step(b, it)
    # checkpoint in the reference's ckpt.tar format, resume in a NEW renderer / trainer
    path = os.path.join(args.out, "ckpt.tar")
    torch.save(trainer.save_checkpoint(half), path)
    renderer2 = EndoSurfRenderer(B.render_cfg(cfg), dict(B.NET_CFG), device=dev)
    trainer2 = Trainer(renderer2, n_iter=args.iters, warm_up_end=max(args.iters // 10, 1))
    start = trainer2.load_checkpoint(torch.load(path, weights_only=False))
    assert start == half + 1
    for it in range(start, args.iters + 1):
        b = {k: torch.from_numpy(v).to(dev) for k, v in sched[it - 1].items()}
        trainer2.update_learning_rate(it)
        loss, terms, _ = trainer2.train_step(b, it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    with torch.no_grad():
        e = renderer2(ev["rays"], iter_step=args.iters, perturb_overwrite=False)
    psnr = float(cal_psnr(e["color_map"], ev["color"], ev["mask"]))
    print(f"{args.iters} iterations x {args.rays} rays in {dt:.1f} s ({args.iters * args.rays / dt:.0f} rays/s incl. host data prep), "
          f"final loss {float(loss):.4f}, eval PSNR {psnr:.2f} dB")
    # a full 640x512 frame through the hipGraph-replayed chunk renderer
    from endosurf_amd.trainer import SyntheticScene
    frame_rays = SyntheticScene(dev).frame(t=0.5)
    t1 = time.perf_counter()
    img = renderer2.render_frames(frame_rays, iter_step=args.iters, ray_chunk=2048, perturb_overwrite=False)
    torch.cuda.synchronize()
    print(f"frame 640x512: {time.perf_counter() - t1:.2f} s (first call captures the graph), colour {tuple(img['color'].shape)}, "
          f"depth range {float(img['depth'].min()):.2f}..{float(img['depth'].max()):.2f}")
    np.save(os.path.join(args.out, "frame_color.npy"), img["color"].reshape(512, 640, 3).cpu().numpy().astype(np.float16))
    # observed-space mesh at t = 0.5 (field sampled on the GPU; PyMCubes if installed, else marching tetrahedra)
    v, f = renderer2.extract_observation_geometry(torch.tensor([0.5]), [-1, -1, -1], [1, 1, 1], resolution=96)
    print(f"mesh: {len(v)} vertices, {len(f)} triangles")
    # the same surface without leaving the GPU: welded mesh, analytic normals, colours seen from a point in front of the scene
    t1 = time.perf_counter()
    m = renderer2.extract_observation_mesh(torch.tensor([0.5]), [-1, -1, -1], [1, 1, 1], resolution=256, view_point=[0.0, 0.0, -1.5], refine_steps=1,
                                           band=True, method=args.mesh_method)          # the SDF is queried near the surface only
    torch.cuda.synchronize()
    print(f"on-device mesh at 256^3: {m['vertices'].shape[0]} vertices, {m['triangles'].shape[0]} triangles, median |sdf| at the vertices "
          f"{float(m['sdf'].abs().median()) if m['sdf'].numel() else 0.0:.2e}, {time.perf_counter() - t1:.2f} s")
    st = m["stats"]
    print(f"narrow band: {st['evaluated_points']} of {st['dense_points']} grid points queried ({100.0 * st['evaluated_points'] / st['dense_points']:.1f} %), "
          f"{st['active_blocks']} of {st['blocks']} blocks ({st['seed_blocks']} seeds, {st['rounds']} growth rounds), fallback {st['fallback']}")
    # the demo's 3D number: drop the floaters, then the mean distance from a depth frame's pixels to the nearest mesh vertex.  The depth
    # frame is the synthetic scene's own (tests/synth_scene.py: a sphere of radius 0.55 + 0.08 sin(2 pi t) around (0, 0, 0.05 t))
    clean = renderer2.extract_observation_mesh(torch.tensor([0.5]), [-1, -1, -1], [1, 1, 1], resolution=256, band=True, components=0.9,
                                               method=args.mesh_method)
    K = torch.tensor([[800.0, 0, 319.5, 0], [0, 800.0, 255.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pose = torch.eye(4)
    pose[2, 3] = -1.5
    ys, xs = torch.meshgrid(torch.arange(512.0), torch.arange(640.0), indexing="ij")
    d = torch.stack([(xs - 319.5) / 800.0, (ys - 255.5) / 800.0, torch.ones_like(xs)], -1)          # z-depth s: point = o + s d
    o, c, rad = torch.tensor([0.0, 0.0, -1.5]), torch.tensor([0.0, 0.0, 0.025]), 0.55
    a, b, cc = (d * d).sum(-1), (d * (o - c)).sum(-1), float(((o - c) ** 2).sum()) - rad * rad
    disc = b * b - a * cc
    depth = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / a, torch.zeros_like(b))
    err = renderer2.geometric_error(clean, depth, K, pose, depth_trunc=3.0)
    # ... and the same cloud against the mesh's surface (the closest point of the closest triangle): it does not move with the tessellation
    surf = renderer2.surface_error(clean, depth, K, pose, depth_trunc=3.0, thresholds=(0.01,))
    cs = clean["components"]
    print(f"cleaned mesh: {cs['kept_triangles']} of {m['triangles'].shape[0]} triangles in the largest of {cs['components']} components "
          f"({cs['rounds']} rounds); geometric error against the scene's depth frame: {err:.4f} (to the vertices), "
          f"{surf['mean']:.4f} (to the surface; rmse {surf['rmse']:.4f}, {100.0 * surf['within'][0]:.1f} % within 0.01)")
    # the demo's "Mesh / Texture / Normal" panels of that mesh, without a display: rasterised once on the device, shaded three times
    clean = renderer2.extract_observation_mesh(torch.tensor([0.5]), [-1, -1, -1], [1, 1, 1], resolution=256, view_point=[0.0, 0.0, -1.5], band=True,
                                               components=0.9, method=args.mesh_method)
    t1 = time.perf_counter()
    pics = renderer2.render_mesh(clean, K, pose, 512, 640, view_point=[0.0, 0.0, -1.5])
    torch.cuda.synchronize()
    from endosurf_amd.data import to8b
    for name in ("geometry", "color", "normal"):
        np.save(os.path.join(args.out, f"mesh_{name}.npy"), to8b(pics[name]))
    np.save(os.path.join(args.out, "mesh_depth.npy"), pics["depth"].cpu().numpy())
    from endosurf_amd.data import write_png
    for name in ("geometry", "color", "normal"):
        write_png(os.path.join(args.out, f"mesh_{name}.png"), to8b(pics[name]))
    wrote = "npy + png"
    de = renderer2.mesh_depth_error(clean, depth, depth > 0, K, pose)
    print(f"mesh panels 640x512 ({wrote}) in {1e3 * (time.perf_counter() - t1):.1f} ms: {pics['stats']['covered_pixels']} pixels covered by "
          f"{pics['stats']['work_items']} work items; mesh depth against the scene's depth frame: rmse {de['rmse']:.4f}, coverage {de['coverage']:.3f}")
    # the reference's eval() of that frame, on the device: PSNR / SSIM / depth RMSE against the synthetic scene's own picture of the sphere
    # (a flat grey ball: the numbers say how far the toy training got, not more) and the five-panel sheet as a file
    hit = (depth > 0).float()[None, ..., None].to(dev)
    gt_color = (0.5 * hit).expand(1, 512, 640, 3).contiguous()
    gt_depth = depth[None, ..., None].to(dev).contiguous()
    t1 = time.perf_counter()
    ev = renderer2.evaluate_frames(frame_rays.reshape(1, 512, 640, 9), gt_color, gt_depth, hit, hit, pose[None], depth_max=3.0, iter_step=args.iters,
                                   perturb_overwrite=False)
    write_png(os.path.join(args.out, "eval_000.png"), ev["sheet"][0])
    print(f"eval sheet 3200x512 (eval_000.png) in {time.perf_counter() - t1:.2f} s with the render: " + ", ".join(f"{k} {x:.4f}" for k, x in ev["stats"].items()))
    # the demo's 3D deliverable: NNN_geometry / _color / _normal.ply of the cleaned, grid-clustered mesh and NNN_gt.ply, the depth frame's
    # point cloud with the frame's colours -- packed on the device, written without Open3D
    from endosurf_amd.data import depth_points, read_ply, write_ply
    t1 = time.perf_counter()
    ex = renderer2.export_observation_mesh(os.path.join(args.out, "000"), torch.tensor([0.5]), [-1, -1, -1], [1, 1, 1], resolution=256,
                                           view_point=[0.0, 0.0, -1.5], components=0.9, simplify="grid", band=True, method=args.mesh_method)
    gt = depth_points(depth.to(dev), K, pose, 3.0)
    write_ply(os.path.join(args.out, "000_gt.ply"), gt, colors=gt_color[0][(depth > 0).to(dev)], engine=renderer2.engine)
    torch.cuda.synchronize()
    back = read_ply(ex["paths"]["normal"])
    print(f"mesh files 000_geometry / _color / _normal / _gt.ply in {time.perf_counter() - t1:.2f} s with the extraction: "
          f"{back['triangles'].shape[0]} triangles of {m['triangles'].shape[0]} ({ex['simplify']['cells']} cells, {ex['clean']['duplicates']} duplicates "
          f"and {ex['clean']['degenerate']} degenerate triangles removed before clustering), {gt.shape[0]} ground-truth points")
    assert np.isfinite(psnr) and len(v) > 0 and m["vertices"].shape[0] > 0 and back["triangles"].shape[0] > 0


if __name__ == "__main__":
    main()
