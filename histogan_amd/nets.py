"""HistoGAN networks on the MI355X kernels: same classes, constructor arguments, forward signatures and
state_dict key names as histoGAN/histoGAN.py of the reference (so its checkpoints load), different
execution plan:

* Conv2DMod (reference :404-440) runs in activation-modulation form
      out = d[b,o] * conv(up?(x) * (s+1), W),   d = rsqrt(((s+1)^2) @ sum_k W^2 + 1e-8)
  -- prologue/epilogue are the fused HIP kernels of histogan_amd/csrc/hg_nets.hip, the dense contraction
  is the hand-written fp32-MFMA implicit GEMM of histogan_amd/csrc/hg_conv.hip on the SHARED weight
  (no B x O x I x k x k per-sample weights, no grouped conv, no MIOpen).
* GeneratorBlock (reference :443-502) fuses the bilinear x2 upsample into conv1's prologue and the
  noise add + LeakyReLU(0.2) (+ demodulation) into each conv's epilogue.
* Discriminator (reference :505-631): every convolution (3x3, 1x1, 3x3 stride 2) runs on the same MFMA
  implicit-GEMM kernels through autograd Functions that are differentiable to any order (convolutions; the grouped style projections, the fused generator stage and the modulation / epilogue kernels are first order: ops.py) (the gradient
  penalty, reference :156-163, needs the second); LeakyReLU / residual add / Linear stay torch ops.
"""
import os
from math import log2

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .conv import conv2d, conv2d_add, conv2d_lrelu, conv2d_same

EPS = 1e-8  # histoGAN/histoGAN.py:53


def leaky_relu(p=0.2):
    return nn.LeakyReLU(p, inplace=True)


class Flatten(nn.Module):
    def forward(self, x):
        return x.reshape(x.shape[0], -1)


def _noise_t(inoise):
    """(B,S,S,1) noise image -> (B,S,S) transposed copy.  A noise image that requires grad (projection: the optimiser's
    variable) is transposed inside the autograd graph, which transposes its gradient back, and is not cached.  Any other
    is cached on the tensor for the G forward, keyed on the tensor's version counter: an in-place update invalidates it."""
    if inoise.requires_grad:
        return inoise[..., 0].transpose(1, 2).contiguous()
    try:
        version = inoise._version
    except Exception:                     # (inference tensors keep no version counter: nothing to key a cache on)
        return inoise[..., 0].transpose(1, 2).contiguous()
    ent = getattr(inoise, '_hg_nzt', None)
    if ent is not None and ent[0] == version:
        return ent[1]
    nzt = inoise[..., 0].transpose(1, 2).contiguous()
    try:
        inoise._hg_nzt = (version, nzt)
    except Exception:
        pass
    return nzt


PHASE_HOOK = None     # tools/phase_probe.py: called with a phase name at points inside the networks (None: no-op)
_aux_streams = {}


def aux_stream(device):
    """A second stream for small launches that only depend on the latents (style projections, the histogram vectorizer)."""
    st = _aux_streams.get(device.index)
    if st is None:
        st = _aux_streams[device.index] = torch.cuda.Stream(device=device)
    return st


class Conv2DMod(nn.Module):
    def __init__(self, in_chan, out_chan, kernel, demod=True, stride=1, dilation=1, **kwargs):
        super().__init__()
        self.filters = out_chan
        self.demod = demod
        self.kernel = kernel
        self.stride = stride
        self.dilation = dilation
        self.weight = nn.Parameter(torch.randn((out_chan, in_chan, kernel, kernel)))
        nn.init.kaiming_normal_(self.weight, a=0, mode='fan_in', nonlinearity='leaky_relu')

    def _get_same_padding(self, size, kernel, dilation, stride):
        return ((size - 1) * (stride - 1) + dilation * (kernel - 1)) // 2

    def demod_coeff(self, y):
        """d[b,o] = rsqrt(sum_{i,k} (W[o,i,k] (y[b,i]+1))^2 + EPS)   (reference :427-429)."""
        return ops.demod_coeff(y, self.weight)        # (GPU only, like every op of this module: CPU tensors raise)

    def contract(self, x, y, upsample=False):
        """conv(up?(x) * (y+1), W): the dense part, shared weights."""
        if self.stride != 1:
            raise NotImplementedError('Conv2DMod: stride != 1 is not used by HistoGAN and not implemented')
        xm = ops.modulate(x, y, upsample)
        if self.dilation == 1 and self.kernel in (1, 3):
            return conv2d_same(xm, self.weight)      # fp32-MFMA implicit GEMM (include/hg_conv.h)
        raise NotImplementedError('Conv2DMod: only 1x1 / 3x3, dilation 1 (all HistoGAN uses) is implemented')

    def forward(self, x, y):
        c = self.contract(x, y)
        if self.demod:
            c = c * self.demod_coeff(y)[:, :, None, None]
        return c


class RGBBlock(nn.Module):
    def __init__(self, latent_dim, input_channel, upsample, rgba=False):
        super().__init__()
        self.input_channel = input_channel
        self.to_style = nn.Linear(latent_dim, input_channel)
        out_filters = 3 if not rgba else 4
        self.conv = Conv2DMod(input_channel, out_filters, 1, demod=False)
        # kept for state_dict/attribute parity; the HIP upsample kernel is used in forward
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) if upsample else None

    def forward(self, x, prev_rgb, istyle):
        return self.forward_(x, prev_rgb, self.to_style(istyle))

    def forward_(self, x, prev_rgb, style):
        if (not self.conv.demod and self.conv.kernel == 1 and self.conv.stride == 1 and self.conv.dilation == 1
                and ops.torgb_supported(x, self.conv.weight) and style.dtype == torch.float32):
            # the 1x1 modulated convolution onto 3 channels + the running RGB image as one stream over x (ops._ToRGB)
            x = ops.torgb(x, style, self.conv.weight, prev_rgb)
            return ops.upsample2x(x) if self.upsample is not None else x
        if GeneratorBlock._fused() and x.is_cuda and not self.conv.demod and self.conv.kernel == 1:
            x = ops.modconv_stage(x, style, self.conv.weight, demod=False, upsample=False, act=False)
        else:
            x = self.conv(x, style)
        if prev_rgb is not None:
            x = x + prev_rgb
        if self.upsample is not None:
            x = ops.upsample2x(x)
        return x


class GeneratorBlock(nn.Module):
    def __init__(self, latent_dim, input_channels, filters, upsample=True, upsample_rgb=True, rgba=False):
        super().__init__()
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) if upsample else None
        self.to_style1 = nn.Linear(latent_dim, input_channels)
        self.to_noise1 = nn.Linear(1, filters)
        self.conv1 = Conv2DMod(input_channels, filters, 3)
        self.to_style2 = nn.Linear(latent_dim, filters)
        self.to_noise2 = nn.Linear(1, filters)
        self.conv2 = Conv2DMod(filters, filters, 3)
        self.activation = leaky_relu()
        self.to_rgb = RGBBlock(latent_dim, filters, upsample_rgb, rgba)

    # Execution plan of one convolution stage.  FUSED = True runs modulation + convolution + demodulation + noise +
    # LeakyReLU as ONE forward launch (ops.modconv_stage -> hg_modconv2d_fwd).  Measured on MI355X at the C3 shapes
    # (tools/modconv_probe.py) the fused forward saves 0.03-0.17 ms per stage but its backward needs the modulation
    # inside the weight-gradient kernel (+0.06-0.1 ms), so the train step is 1-3 % faster with the three-kernel
    # plan below (prologue kernel, convolution, epilogue kernel).  Without autograd (the D phase's generator forward,
    # evaluate()) there is no backward to pay for, so the fused launch is used there whatever FUSED says.
    FUSED = False

    @classmethod
    def _fused(cls):
        return cls.FUSED or not torch.is_grad_enabled()

    def _stage(self, conv, x, style, nzt, to_noise, upsample):
        if self._fused() and conv.stride == 1 and conv.dilation == 1 and conv.kernel in (1, 3):
            return ops.modconv_stage(x, style, conv.weight, nzt, to_noise.weight, to_noise.bias,
                                     demod=conv.demod, upsample=upsample, act=True)
        # (d before the convolution: the backward then reaches the convolution's weight gradient first, which writes the flat
        # gradient slot outright, and the demodulation's weight term accumulates into it -- conv.direct_weight_term)
        d = conv.demod_coeff(style) if conv.demod else None
        if (conv.stride == 1 and conv.dilation == 1 and conv.kernel in (1, 3) and x.is_cuda
                and nzt.shape[-1] % 2 == 0 and conv.weight.dtype == torch.float32):
            # modulation prologue (materialised: the weight gradient's operand), then convolution + demodulation + noise +
            # LeakyReLU as one launch (ops._ConvDnl)
            return ops.conv_dnl(ops.modulate(x, style, upsample), conv.weight, d, nzt, to_noise.weight, to_noise.bias)
        c = conv.contract(x, style, upsample)
        return ops.demod_noise_lrelu(c, d, nzt, to_noise.weight, to_noise.bias)

    def forward(self, x, prev_rgb, istyle, inoise, latent=None):
        return self.forward_(x, prev_rgb, self.to_style1(istyle), self.to_style2(istyle),
                             self.to_rgb.to_style(istyle), inoise=inoise, latent=latent)

    def forward_(self, x, prev_rgb, style1, style2, to_rgb_style, inoise=None, noise1=None, noise2=None,
                 latent=None):
        if noise1 is not None and noise2 is not None:
            # explicit per-pixel noise tensors (projection scripts): unfused path, same maths
            if self.upsample is not None:
                x = ops.upsample2x(x)
            x = F.leaky_relu(self.conv1(x, style1) + noise1, 0.2)
            if latent is not None:
                x = x + latent
            x = F.leaky_relu(self.conv2(x, style2) + noise2, 0.2)
            return x, self.to_rgb.forward_(x, prev_rgb, to_rgb_style)
        if inoise is None:
            raise Exception('No noise is given')
        nzt = _noise_t(inoise)
        x = self._stage(self.conv1, x, style1, nzt, self.to_noise1, self.upsample is not None)
        if latent is not None:
            x = x + latent
        x = self._stage(self.conv2, x, style2, nzt, self.to_noise2, False)
        return x, self.to_rgb.forward_(x, prev_rgb, to_rgb_style)


class Generator(nn.Module):
    def __init__(self, image_size, latent_dim, network_capacity=16, transparent=False):
        super().__init__()
        self.image_size = image_size
        self.latent_dim = latent_dim
        self.num_layers = int(log2(image_size) - 1)
        init_channels = 4 * network_capacity
        self.initial_block = nn.Parameter(torch.randn((init_channels, 4, 4)))
        filters = [init_channels] + [network_capacity * (2 ** (i + 1)) for i in range(self.num_layers)][::-1]
        self.blocks = nn.ModuleList([])
        for ind, (in_chan, out_chan) in enumerate(zip(filters[0:-1], filters[1:])):
            self.blocks.append(GeneratorBlock(latent_dim, in_chan, out_chan, upsample=ind != 0,
                                              upsample_rgb=ind != (self.num_layers - 1), rgba=transparent))

    def forward(self, styles, hists, input_noise):
        batch_size = styles.shape[0]
        x = self.initial_block.expand(batch_size, -1, -1, -1)
        styles = torch.cat((styles.transpose(0, 1), hists.transpose(0, 1)), dim=0)
        rgb = None
        layers = [m for block in self.blocks for m in (block.to_style1, block.to_style2, block.to_rgb.to_style)]
        if (styles.dtype == torch.float32 and styles.shape[0] >= len(self.blocks)     # (fewer style rows than blocks: the zip below)
                and ops.grouped_linear_supported([styles[0]], [m.weight for m in layers])):
            # The 21 style projections (three nn.Linear(512, C) per block on the block's style vector) as ONE launch
            # (include/hg_linear.h) instead of 21 library GEMMs of 32 ... 64 workgroups -- and 3 launches instead of 42 GEMMs +
            # 21 bias reductions + the gradient sums in the backward.  Without autograd they still run beside the head of the
            # chain on the second stream.
            groups = [i for i in range(len(self.blocks)) for _ in range(3)]
            xs = [styles[i] for i in range(len(self.blocks))]
            ahead = not torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing()
            if ahead:
                main, aux = torch.cuda.current_stream(styles.device), aux_stream(styles.device)
                aux.wait_event(main.record_event())
                with torch.cuda.stream(aux):
                    t = ops.grouped_linear(xs, layers, groups)
                main.wait_stream(aux)
                for u in t:
                    u.record_stream(main)
                styles.record_stream(aux)
            else:
                t = ops.grouped_linear(xs, layers, groups)
            if PHASE_HOOK is not None:
                PHASE_HOOK('g_styles_projected', False)
            if input_noise is not None and input_noise.dim() == 4:
                from . import gfused
                nzt = _noise_t(input_noise)
                if gfused.supported(self, t, nzt):
                    # training: the whole network as ONE autograd node with a hand-written backward (gfused.py)
                    return gfused.generator_train(self, t, nzt)
                if gfused.supported(self, t, nzt, train=False):
                    return gfused.generator_infer(self, t, nzt)
            for i, block in enumerate(self.blocks):
                x, rgb = block.forward_(x, rgb, t[3 * i], t[3 * i + 1], t[3 * i + 2], inoise=input_noise)
            return rgb
        if styles.is_cuda and not torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing():
            # Without autograd (the D phase's generator forward, evaluate()): the 21 `to_style` projections depend on the
            # styles only, yet as launches between the convolutions each one holds the convolution chain up for a
            # ~15 us GEMM.  They run ahead on a second stream, block by block; the chain waits for its block's event.
            main, aux = torch.cuda.current_stream(styles.device), aux_stream(styles.device)
            aux.wait_event(main.record_event())
            ahead = []
            with torch.cuda.stream(aux):
                for style, block in zip(styles, self.blocks):
                    t = (block.to_style1(style), block.to_style2(style), block.to_rgb.to_style(style))
                    ahead.append((t, aux.record_event()))
            for (t, ev), block in zip(ahead, self.blocks):
                main.wait_event(ev)
                for u in t:
                    u.record_stream(main)
                x, rgb = block.forward_(x, rgb, t[0], t[1], t[2], inoise=input_noise)
            styles.record_stream(aux)
            return rgb
        for style, block in zip(styles, self.blocks):
            x, rgb = block(x, rgb, style, input_noise)
        return rgb


class HistVectorizer(nn.Module):
    def __init__(self, insize, emb, depth):
        super().__init__()
        self.flatten = Flatten()
        fc_layers = []
        for i in range(depth):
            if i == 0:
                fc_layers.extend([nn.Linear(insize * insize * 3, emb * 2), leaky_relu()])
            elif i == 1:
                fc_layers.extend([nn.Linear(emb * 2, emb), leaky_relu()])
            else:
                fc_layers.extend([nn.Linear(emb, emb), leaky_relu()])
        self.fcs = nn.Sequential(*fc_layers)

    def forward(self, x):
        x = self.flatten(x)
        if x.is_cuda and ops.SKINNY_SPLIT and len(self.fcs) >= 2 and x.shape[0] <= 64:
            # the first layer is a (B x 12288) @ (12288 x 1024) product with B = 32: rocBLAS runs it as 16 x 256 tiles with no
            # split over the 12288-deep reduction, 102 us at the start of every generator forward; as chunks of the reduction
            # (ops._skinny_mm: a strided bmm + a sum) it is ~4x the workgroups
            fc = self.fcs[0]
            h = ops._skinny_mm(x.contiguous(), fc.weight, True)
            if fc.bias is not None:
                h = h + fc.bias
            return self.fcs[1:](h)
        return self.fcs(x)


class StyleVectorizer(nn.Module):
    def __init__(self, emb, depth):
        super().__init__()
        layers = []
        for i in range(depth):
            layers.extend([nn.Linear(emb, emb), leaky_relu()])
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return self.net(x)


class Conv2d(nn.Conv2d):
    """nn.Conv2d (same parameters, init and state_dict keys) whose forward runs on the MFMA implicit-GEMM
    kernels: 1x1 / 3x3, stride 1 or 2, padding k//2 -- every convolution of the discriminator (:510-518)."""

    def forward(self, x):
        k = self.kernel_size[0]
        if (self.kernel_size[0] != self.kernel_size[1] or self.padding != (k // 2, k // 2) or self.dilation != (1, 1)
                or self.groups != 1 or self.stride[0] != self.stride[1] or self.padding_mode != 'zeros'):
            raise NotImplementedError('Conv2d: only square 1x1/3x3, padding k//2, stride 1/2, dilation 1, groups 1')
        return conv2d(x, self.weight, self.bias, self.stride[0])


class DiscriminatorBlock(nn.Module):
    def __init__(self, input_channels, filters, downsample=True):
        super().__init__()
        self.conv_res = Conv2d(input_channels, filters, 1)
        self.net = nn.Sequential(Conv2d(input_channels, filters, 3, padding=1), leaky_relu(),
                                 Conv2d(filters, filters, 3, padding=1), leaky_relu())
        self.downsample = Conv2d(filters, filters, 3, padding=1, stride=2) if downsample else None

    def forward(self, x):
        # conv + bias + LeakyReLU(0.2) as one launch each (== self.net(x): Conv2d, LeakyReLU, Conv2d, LeakyReLU), and the
        # residual sum `net(x) + conv_res(x)` in the epilogue of the 1x1 conv_res launch (same value: (conv + bias) + h)
        h = conv2d_lrelu(x, self.net[0].weight, self.net[0].bias, 0.2)
        h = conv2d_lrelu(h, self.net[2].weight, self.net[2].bias, 0.2)
        x = conv2d_add(x, self.conv_res.weight, self.conv_res.bias, h)
        if self.downsample is not None:
            x = self.downsample(x)
        return x


class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x) + x


class Rezero(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn
        self.g = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return self.fn(x) * self.g


class ImageLinearAttention(nn.Module):
    """Linear attention over the pixels of a feature map, the discriminator's optional `attn_layers`
    (reference histoGAN/histoGAN.py:594-596 imports it from the third-party `linear_attention_transformer`, whose source
    is NOT in the reference tree and whose version is unpinned: restated from the published algorithm -- Shen et al.,
    "Efficient Attention", as implemented in that package's images.py -- PARITY UNPINNED).

        q, k, v = 1x1 convs of x -> (b, heads, d, n), n = h*w;   q, k *= d^-1/4
        k = softmax over n;  q = softmax over d (norm_queries);  ctx = k v^T (d x e per head);  out = ctx^T q -> 1x1 conv

    The four 1x1 convolutions run on the MFMA kernels (differentiable to any order: the gradient penalty goes through
    them), the two softmaxes and the two small batched GEMMs (d = e = 64) are torch / rocBLAS ops."""

    def __init__(self, chan, chan_out=None, kernel_size=1, padding=0, stride=1, key_dim=64, value_dim=64, heads=8,
                 norm_queries=True):
        super().__init__()
        if kernel_size != 1 or padding != 0 or stride != 1:
            raise NotImplementedError('ImageLinearAttention: only the 1x1 projections HistoGAN uses')
        self.chan = chan
        chan_out = chan if chan_out is None else chan_out
        self.key_dim, self.value_dim, self.heads, self.norm_queries = key_dim, value_dim, heads, norm_queries
        self.to_q = Conv2d(chan, key_dim * heads, 1)
        self.to_k = Conv2d(chan, key_dim * heads, 1)
        self.to_v = Conv2d(chan, value_dim * heads, 1)
        self.to_out = Conv2d(value_dim * heads, chan_out, 1)

    def forward(self, x, context=None):
        if context is not None:
            raise NotImplementedError('ImageLinearAttention: cross-attention context is not used by HistoGAN')
        b, c, h, w = x.shape
        heads = self.heads
        q, k, v = self.to_q(x), self.to_k(x), self.to_v(x)
        q, k, v = (t.reshape(b, heads, -1, h * w) for t in (q, k, v))
        q, k = (t * (self.key_dim ** -0.25) for t in (q, k))
        k = k.softmax(dim=-1)
        if self.norm_queries:
            q = q.softmax(dim=-2)
        context = torch.einsum('bhdn,bhen->bhde', k, v)
        out = torch.einsum('bhdn,bhde->bhen', q, context)
        return self.to_out(out.reshape(b, -1, h, w))


class PermuteToFrom(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        out, loss = self.fn(x.permute(0, 2, 3, 1))
        return out.permute(0, 3, 1, 2), loss


class VectorQuantize(nn.Module):
    """Feature quantisation of the discriminator's optional `fq_layers` (reference histoGAN/histoGAN.py:598-600 takes it
    from the third-party `vector_quantize_pytorch`, absent from the reference tree and unpinned: restated from the
    published algorithm -- VQ-VAE codebook with exponential-moving-average updates, straight-through estimator and
    commitment loss -- PARITY UNPINNED).  Buffers `embed` (dim, n_embed), `cluster_size`, `embed_avg` as upstream.
    Nearest-code search and the EMA statistics are two small GEMMs (rocBLAS); under data parallelism the statistics are
    all-reduced (counts and sums of the global batch) and the buffers broadcast at init / after load, so every replica
    holds the same codebook (the reference is single-GPU)."""

    def __init__(self, dim, n_embed, decay=0.8, commitment=1., eps=1e-5):
        super().__init__()
        self.dim, self.n_embed, self.decay, self.commitment, self.eps = dim, n_embed, decay, commitment, eps
        embed = torch.randn(dim, n_embed)
        self.register_buffer('embed', embed)
        self.register_buffer('cluster_size', torch.zeros(n_embed))
        self.register_buffer('embed_avg', embed.clone())

    def forward(self, input):
        flatten = input.reshape(-1, self.dim)
        dist = flatten.pow(2).sum(1, keepdim=True) - 2 * flatten @ self.embed + self.embed.pow(2).sum(0, keepdim=True)
        embed_ind = (-dist).max(1)[1]
        quantize = F.embedding(embed_ind.view(*input.shape[:-1]), self.embed.transpose(0, 1))
        if self.training:
            with torch.no_grad():
                onehot = F.one_hot(embed_ind, self.n_embed).type(input.dtype)
                counts, sums = onehot.sum(0), flatten.detach().transpose(0, 1) @ onehot
                from . import ddp
                if ddp.is_dist():            # the codebook statistics of the GLOBAL batch: replicas keep identical codebooks
                    packed = torch.cat([counts.reshape(1, -1), sums], dim=0)
                    torch.distributed.all_reduce(packed)
                    counts, sums = packed[0], packed[1:]
                self.cluster_size.mul_(self.decay).add_(counts, alpha=1 - self.decay)
                self.embed_avg.mul_(self.decay).add_(sums, alpha=1 - self.decay)
                n = self.cluster_size.sum()
                cluster_size = (self.cluster_size + self.eps) / (n + self.n_embed * self.eps) * n     # Laplace smoothing
                self.embed.copy_(self.embed_avg / cluster_size.unsqueeze(0))
        loss = F.mse_loss(quantize.detach(), input) * self.commitment
        quantize = input + (quantize - input).detach()
        return quantize, loss


class Discriminator(nn.Module):
    def __init__(self, image_size, network_capacity=16, fq_layers=[], fq_dict_size=256, attn_layers=[],
                 transparent=False):
        super().__init__()
        num_layers = int(log2(image_size) - 1)
        num_init_filters = 3 if not transparent else 4
        filters = [num_init_filters] + [network_capacity * (2 ** i) for i in range(num_layers + 1)]
        chan_in_out = list(zip(filters[0:-1], filters[1:]))
        self.blocks = nn.ModuleList([DiscriminatorBlock(i, o, downsample=ind != (len(chan_in_out) - 1))
                                     for ind, (i, o) in enumerate(chan_in_out)])
        attn_layers = [int(a) for a in attn_layers]
        self.attn_blocks = nn.ModuleList([
            nn.Sequential(*[Residual(Rezero(ImageLinearAttention(o))) for _ in range(2)])
            if ind + 1 in attn_layers else None for ind, (i, o) in enumerate(chan_in_out)])
        fq_layers = [int(a) for a in fq_layers]
        self.quantize_blocks = nn.ModuleList([
            PermuteToFrom(VectorQuantize(o, fq_dict_size)) if ind + 1 in fq_layers else None
            for ind, (i, o) in enumerate(chan_in_out)])
        self.flatten = Flatten()
        self.to_logit = nn.Linear(2 * 2 * filters[-1], 1)

    def forward(self, x):
        quantize_loss = torch.zeros(1, device=x.device, dtype=x.dtype)
        for block, attn_block, q_block in zip(self.blocks, self.attn_blocks, self.quantize_blocks):
            x = block(x)
            if attn_block is not None:
                x = attn_block(x)
            if q_block is not None:
                x, loss = q_block(x)
                quantize_loss = quantize_loss + loss
        x = self.flatten(x)
        if x.is_cuda and ops.SKINNY_SPLIT and self.to_logit.out_features == 1:
            # (B x 8192) @ (8192 x 1): rocBLAS runs the logit layer as ONE workgroup walking the whole reduction, 100 us at the
            # end of every discriminator forward; a product and a row sum are two short memory-bound launches
            x = (x * self.to_logit.weight).sum(dim=1, keepdim=True) + self.to_logit.bias
        else:
            x = self.to_logit(x)
        return x.squeeze(), quantize_loss
