"""Save what env 0 of a batch does as pictures: a short random-action episode of FurnitureBatchEnv with one world camera, the
Lambert-shaded colour-by-part image of the collision geometry (furniture_amd.normals) of every step written as a binary PPM.
  python scripts/save_frames.py OUT_DIR [--agent Sawyer] [--furniture table_lack_0825] [--envs 16] [--steps 30] [--size 256] [--seed 0]
The frames are OUT_DIR/frame_0000.ppm ...; any image viewer or `ffmpeg -i frame_%04d.ppm clip.mp4` reads them."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from furniture_amd.camera import Camera
from furniture_amd.envs import FurnitureBatchEnv, make_config
from furniture_amd.normals import Normals, save_ppm

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("out_dir")
ap.add_argument("--agent", default="Sawyer")
ap.add_argument("--furniture", default="table_lack_0825")
ap.add_argument("--envs", type=int, default=16)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
os.makedirs(a.out_dir, exist_ok=True)
cam = Camera((1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50, width=a.size, height=a.size)
cfg = make_config(unity=False, record_vid=False, furniture_name=a.furniture, seed=a.seed)
env = FurnitureBatchEnv(a.agent, a.envs, config=cfg, cameras=[cam], normals=Normals(normal=False, shaded=True))
rng = np.random.RandomState(a.seed)
ob = env.reset()
for t in range(a.steps + 1):
    save_ppm(os.path.join(a.out_dir, "frame_%04d.ppm" % t), ob["camera_shaded"][0, 0].cpu().numpy())
    if t < a.steps:
        ob, _, _, _ = env.step(rng.uniform(-1, 1, (a.envs, env.dof)).astype(np.float32))
env.close()
print("%d frames of env 0 in %s" % (a.steps + 1, a.out_dir))
