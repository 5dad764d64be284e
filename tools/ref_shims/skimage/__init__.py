"""Import shim for tools/gen_golden.py ONLY (never on the product path, never on the GPU box).

scikit-image is not installed in this image; the reference's post-optimisation imports `skimage.color` for
rgb2lab alone (monodepth/networks/utils/postopt_utils.py:107).  See color.py: parity unpinned, like cv2."""
