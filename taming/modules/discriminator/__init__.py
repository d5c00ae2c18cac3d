"""`taming.modules.discriminator`: the PatchGAN discriminator of the tokenizer's loss."""
