"""Apps that work with a trained generator checkpoint: ``python -m tartangan_amd.explore.{find_image,render_tour,continuous_interp}``."""
