"""Drop-in replacement module for the reference ``inference.py`` (``from inference import
run_unet``, app_camera.py:16)."""
from unet_mi355x.inference import (DEVICE, FIELDS, IMG_SIZE, evaluate, finetune_head, load_model,  # noqa: F401
                                   preprocess, run_unet)
