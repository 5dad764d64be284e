"""Dev-only stand-in for the nuScenes devkit (absent in this image) so that tools/gen_golden.py can run the
reference's nuScenes dataset and evaluator over a tiny seeded tree: NuScenes (JSON tables, get, sample, scene, the
sample['data'] reverse index), LidarPointCloud (from_file, remove_close, transform, nbr_points) and transform_matrix.
This is this project's reading of the devkit and is not pinned against the real one.  Never imported on the product
path or the GPU box."""
