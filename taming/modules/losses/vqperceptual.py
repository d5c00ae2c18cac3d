"""`taming.modules.losses.vqperceptual` (lossconfig.target of every shipped tokenizer config) -> the forward-only HIP implementation."""
from frido_amd.models import (DummyLoss, LPIPS, NLayerDiscriminator, VQLPIPSWithDiscriminator, adopt_weight, hinge_d_loss,  # noqa: F401
                              vanilla_d_loss, weights_init)
