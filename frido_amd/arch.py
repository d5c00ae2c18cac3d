"""Architecture walk of the denoiser and the MS-VQGAN: which blocks exist, in which order, with
which state_dict prefixes and channel counts.  Pure host logic (no tensors); it is what both the
HIP plan builders and the oracle iterate over, and it is pinned by the golden fixtures' key lists.

Restates the constructor loops of the reference:
  frido/modules/diffusionmodules/pyunet.py:575-803   (PyUNetModel.__init__)
  taming/modules/diffusionmodules/model.py:435-510   (MSEncoder.__init__)
  taming/modules/diffusionmodules/model.py:548-616   (Decoder.__init__)
"""
from dataclasses import dataclass, field
from typing import List, Optional

__all__ = ["UNetArch", "unet_arch", "DecoderArch", "decoder_arch", "EncoderArch", "encoder_arch", "MH_HEAD_DIMS",
           "check_attention_heads"]

# head dimensions the multi-head flash kernel (csrc/flash_mh.hip) is instantiated for; the library answers the same through
# frido_attn_mh_supported (tests compare the two).  Kept here so that a model is refused at construction, before any library is loaded.
MH_HEAD_DIMS = (32, 64)


def check_attention_heads(heads, d, where="attention"):
    """Raise NotImplementedError for a (heads, head dim) pair no kernel serves: one head takes the single-head kernels (any d that is
    a multiple of 32), several heads need d in MH_HEAD_DIMS."""
    if heads > 1 and d not in MH_HEAD_DIMS:
        raise NotImplementedError(f"{where}: {heads} heads of {d} channels -- the multi-head attention kernel is built for head "
                                  f"dimensions {', '.join(map(str, MH_HEAD_DIMS))} only (one head: any multiple of 32)")


@dataclass
class Blk:
    kind: str            # 'res' | 'st' | 'attn' | 'down' | 'up'
    prefix: str          # state_dict prefix relative to the U-Net root, e.g. 'input_blocks.3.0'
    cin: int
    cout: int
    heads: int = 1       # 'attn' (AttentionBlock, pyunet.py:303-358): number of heads of cin / heads channels ...
    new_order: bool = False      # ... and whether qkv is split before the heads (QKVAttention) or after (QKVAttentionLegacy)


@dataclass
class UNetArch:
    model_channels: int
    time_embed_dim: int
    context_dim: Optional[int]
    num_stage: int
    splits: List[int]
    use_spade: bool
    use_split_head: bool
    in_channels: int
    input_blocks: List[List[Blk]] = field(default_factory=list)
    middle: List[Blk] = field(default_factory=list)
    output_blocks: List[List[Blk]] = field(default_factory=list)
    skip_channels: List[int] = field(default_factory=list)   # channels pushed on the skip stack
    image_size: int = 64
    transformer_depth: int = 1     # BasicTransformerBlocks per SpatialTransformer (attention.py:274-277)
    num_classes: Optional[int] = None      # class-conditional denoiser: label_emb (pyunet.py:567-571) ...
    use_embed: bool = False                # ... nn.Embedding (y int64 [B]) or nn.Linear (y float [B, num_classes])

    def attention_sites(self):
        """Every 'st' / 'attn' block in forward order."""
        return [blk for grp in (self.input_blocks + [self.middle] + self.output_blocks) for blk in grp if blk.kind in ("st", "attn")]


def unet_arch(cfg) -> UNetArch:
    mc = cfg["model_channels"]
    mult = list(cfg.get("channel_mult", (1, 2, 4, 8)))
    nres = cfg["num_res_blocks"]
    attn_res = set(cfg["attention_resolutions"])
    use_st = cfg.get("use_spatial_transformer", False)
    if cfg.get("resblock_updown", False) or cfg.get("use_scale_shift_norm", False):
        raise NotImplementedError("resblock_updown / use_scale_shift_norm are not used by any Frido config")
    depth = int(cfg.get("transformer_depth", 1))
    if depth < 1:
        raise ValueError("transformer_depth must be >= 1")
    if not use_st and cfg.get("context_dim") is not None:      # pyunet.py:516-517
        raise ValueError("context_dim needs use_spatial_transformer=True: the AttentionBlock denoiser has no cross-attention")
    if use_st and not cfg.get("legacy", True):
        raise NotImplementedError("legacy=False with use_spatial_transformer=True (multi-head SpatialTransformer) is not built")
    a = UNetArch(model_channels=mc, time_embed_dim=4 * mc, context_dim=cfg.get("context_dim"),
                 num_stage=cfg.get("num_stage", 1), splits=list(cfg.get("split_embed_dim_list", [])),
                 use_spade=cfg.get("use_SPADE_norm", False), use_split_head=cfg.get("use_split_head", False),
                 in_channels=cfg["in_channels"], image_size=cfg.get("image_size", 64), transformer_depth=depth,
                 num_classes=cfg.get("num_classes"), use_embed=bool(cfg.get("use_embed", False)))
    # head count of an AttentionBlock site, by the reference's rules: the constructor loops (pyunet.py:633-640, 686-693, 751-758) carry
    # `num_heads` from site to site, legacy=True forces it to 1 and passes num_head_channels through, the output path hands
    # num_heads_upsample to the block, and AttentionBlock.__init__ (323-329) lets a head width override the count
    nh = [cfg.get("num_heads", -1)]
    nhc = cfg.get("num_head_channels", -1)
    nh_up = cfg.get("num_heads_upsample", -1)
    nh_up = nh[0] if nh_up == -1 else nh_up
    legacy = cfg.get("legacy", True)
    new_order = bool(cfg.get("use_new_attention_order", False))

    def attn(prefix, ch, out_path=False):
        if use_st:
            return Blk("st", prefix, ch, ch)
        if nhc == -1:
            dim_head = ch // nh[0]
        else:
            nh[0] = ch // nhc
            dim_head = nhc
        if legacy:
            nh[0] = 1
            dim_head = nhc
        heads = nh_up if out_path else nh[0]
        if dim_head != -1:
            if dim_head <= 0 or ch % dim_head:
                raise ValueError(f"{prefix}: q,k,v channels {ch} is not divisible by num_head_channels {dim_head}")
            heads = ch // dim_head
        if heads < 1 or ch % heads:
            raise ValueError(f"{prefix}: {ch} channels do not split into {heads} heads")
        check_attention_heads(heads, ch // heads, f"AttentionBlock {prefix} ({ch} channels)")
        return Blk("attn", prefix, ch, ch, heads=heads, new_order=new_order)

    # pyunet.py:600-609: with the split head input_blocks starts empty, otherwise block 0 is the conv
    idx = 0 if a.use_split_head else 1
    chans = [mc]
    ch = mc
    ds = 1
    for level, m in enumerate(mult):
        for _ in range(nres):
            blk = [Blk("res", f"input_blocks.{idx}.0", ch, m * mc)]
            ch = m * mc
            if ds in attn_res:
                blk.append(attn(f"input_blocks.{idx}.1", ch))
            a.input_blocks.append(blk)
            chans.append(ch)
            idx += 1
        if level != len(mult) - 1:
            a.input_blocks.append([Blk("down", f"input_blocks.{idx}.0", ch, ch)])
            chans.append(ch)
            idx += 1
            ds *= 2
    a.skip_channels = list(chans)
    a.middle = [Blk("res", "middle_block.0", ch, ch), attn("middle_block.1", ch),
                Blk("res", "middle_block.2", ch, ch)]
    oidx = 0
    for level, m in list(enumerate(mult))[::-1]:
        for i in range(nres + 1):
            ich = chans.pop()
            blk = [Blk("res", f"output_blocks.{oidx}.0", ch + ich, mc * m)]
            ch = mc * m
            j = 1
            if ds in attn_res:
                blk.append(attn(f"output_blocks.{oidx}.{j}", ch, out_path=True))
                j += 1
            if level and i == nres:
                blk.append(Blk("up", f"output_blocks.{oidx}.{j}", ch, ch))
                ds //= 2
            a.output_blocks.append(blk)
            oidx += 1
    return a


# ------------------------------------------------------------------------------------------------
@dataclass
class VBlk:
    kind: str            # 'res' | 'attn' | 'up' | 'down'
    prefix: str
    cin: int
    cout: int


@dataclass
class DecoderArch:
    z_channels: int
    block_in: int
    out_ch: int
    z_res: int
    body: List[VBlk] = field(default_factory=list)   # everything between conv_in and norm_out
    last_ch: int = 0


def decoder_arch(dd, prefix="decoder") -> DecoderArch:
    ch, mult = dd["ch"], list(dd["ch_mult"])
    nres = dd["num_res_blocks"]
    attn_res = set(dd["attn_resolutions"])
    nlev = len(mult)
    block_in = ch * mult[-1]
    res = dd["resolution"] // 2 ** (nlev - 1)
    d = DecoderArch(z_channels=dd["z_channels"], block_in=block_in, out_ch=dd["out_ch"], z_res=res)
    d.body += [VBlk("res", f"{prefix}.mid.block_1", block_in, block_in),
               VBlk("attn", f"{prefix}.mid.attn_1", block_in, block_in),
               VBlk("res", f"{prefix}.mid.block_2", block_in, block_in)]
    for lvl in reversed(range(nlev)):
        bout = ch * mult[lvl]
        for i in range(nres + 1):
            d.body.append(VBlk("res", f"{prefix}.up.{lvl}.block.{i}", block_in, bout))
            block_in = bout
            if res in attn_res:
                d.body.append(VBlk("attn", f"{prefix}.up.{lvl}.attn.{i}", block_in, block_in))
        if lvl != 0:
            d.body.append(VBlk("up", f"{prefix}.up.{lvl}.upsample", block_in, block_in))
            res *= 2
    d.last_ch = block_in
    return d


@dataclass
class EncoderArch:
    ch: int
    in_channels: int
    multiscale: int
    down: List[List[VBlk]] = field(default_factory=list)      # per level: blocks incl. trailing 'down'
    level_out_ch: List[int] = field(default_factory=list)
    heads: List[List[VBlk]] = field(default_factory=list)     # mid_ms[i] blocks
    head_ch: List[int] = field(default_factory=list)
    z_channels: List[int] = field(default_factory=list)


def encoder_arch(ed, prefix="encoder") -> EncoderArch:
    ch, mult = ed["ch"], list(ed["ch_mult"])
    nres = ed["num_res_blocks"]
    attn_res = set(ed["attn_resolutions"])
    ms = ed["multiscale"]
    e = EncoderArch(ch=ch, in_channels=ed["in_channels"], multiscale=ms, z_channels=list(ed["z_channels"]))
    in_mult = [1] + mult
    res = ed["resolution"]
    for lvl in range(len(mult)):
        bin_, bout = ch * in_mult[lvl], ch * mult[lvl]
        blocks = []
        for i in range(nres):
            blocks.append(VBlk("res", f"{prefix}.down.{lvl}.block.{i}", bin_, bout))
            bin_ = bout
            if res in attn_res:
                blocks.append(VBlk("attn", f"{prefix}.down.{lvl}.attn.{i}", bin_, bin_))
        if lvl != len(mult) - 1:
            blocks.append(VBlk("down", f"{prefix}.down.{lvl}.downsample", bin_, bin_))
            res //= 2
        e.down.append(blocks)
        e.level_out_ch.append(bout)
    for i, m in enumerate(in_mult[-ms:]):
        c = ch * m
        e.heads.append([VBlk("res", f"{prefix}.mid_ms.{i}.block_1", c, c),
                        VBlk("attn", f"{prefix}.mid_ms.{i}.attn_1", c, c),
                        VBlk("res", f"{prefix}.mid_ms.{i}.block_2", c, c)])
        e.head_ch.append(c)
    return e
