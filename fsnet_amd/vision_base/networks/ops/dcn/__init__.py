"""Deformable convolution (the classes and functions live in .deform_conv, as in the reference)."""
