"""Writes tests/golden/pose_demo.npz, the real-data fixture of tests/test_pose_ransac.py: two frames from each of the three demo
sequences of the dataset (data/demo/<model>/seq_*/frame_*.npz), 2048 of their 4096 points chosen with a fixed generator.
Data only: the frames' nocs_data / depth_data (f32) and obj_T (f64), with depth ~ obj_T[:3,:3] (nocs - 0.5) + obj_T[:3,3].

    python tests/golden/gen_pose_fixture.py <data/demo directory>"""
import os
import sys

import numpy as np

FRAMES = (0, 7)        # frame positions in each sequence's sorted file list
NUM_PTS = 2048


def main(demo_dir):
    rng = np.random.RandomState(0)
    nocs, depth, pose, names = [], [], [], []
    for model in sorted(os.listdir(demo_dir)):
        for seq in sorted(os.listdir(os.path.join(demo_dir, model))):
            files = sorted(f for f in os.listdir(os.path.join(demo_dir, model, seq)) if f.endswith(".npz"))
            for k in FRAMES:
                d = np.load(os.path.join(demo_dir, model, seq, files[k]))
                pick = np.sort(rng.choice(d["nocs_data"].shape[0], NUM_PTS, replace=False))
                nocs.append(d["nocs_data"][pick].astype(np.float32))
                depth.append(d["depth_data"][pick].astype(np.float32))
                pose.append(d["obj_T"].astype(np.float64))
                names.append("%s/%s/%s" % (model, seq, files[k]))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_demo.npz")
    np.savez_compressed(out, nocs=np.stack(nocs), depth=np.stack(depth), obj_T=np.stack(pose), frames=np.array(names))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
