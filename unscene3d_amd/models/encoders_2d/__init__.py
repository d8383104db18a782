"""2D image encoders of the pseudo-mask generator (reference models/encoders_2d): the DINO ViT-S/8 extractor."""
from .dino import DinoNet, DinoViT

__all__ = ["DinoNet", "DinoViT"]
