"""Weight packing for the conv-stack kernels: everything that turns a (BN-folded) module's weights into the device images the kernels of
csrc/ read (layouts: include/pam.h).  All arithmetic runs on the CPU in float32; an image is rounded to bf16 and moved to the device last.

Three rules are shared by nearly every image and written down once here: the float32 bias (``bias_of``), the MFMA row -> output-channel
permutation (``row_channels``) and the LDS bank swizzle of a row's 16-byte pieces (``swizzle``)."""
import ctypes as C

import torch
import torch.nn as nn


def bias_of(conv, n=None):
    """The float32 bias of a convolution; zeros when it has none (n entries; default: the weight's leading dimension)."""
    if conv.bias is not None:
        return conv.bias.detach().float()
    return torch.zeros(conv.weight.shape[0] if n is None else n)


def bf16_on(t, device):
    return t.to(torch.bfloat16).to(device).contiguous()


def row_channels(group, groups=1):
    """MFMA row -> output channel, for images whose rows are the A operand: rows come in groups of `group` = 16 * nt rows (nt N tiles
    of 16), and row 16 j + q of group g holds channel  group * g + (group / 4) * (q >> 2) + 4 j + (q & 3).  A lane (which owns rows
    q >> 2 == const of every N tile) then ends with group / 4 contiguous output channels: one aligned piece of an output pixel."""
    r = torch.arange(group)
    one = (group // 4) * ((r % 16) >> 2) + 4 * (r // 16) + (r & 3)
    return (group * torch.arange(groups)[:, None] + one[None, :]).reshape(-1)


# the 48-channel kernels (k_bblock2_48, k_down48): N tiles 0, 1 as one group of 32 rows, N tile 2 as a group of 16 -- a lane ends with
# channels 8 g .. 8 g + 7 and 32 + 4 g .. + 3 (aligned 16 + 8 bytes of a pixel)
ROWS48 = torch.cat([row_channels(group=32), 32 + row_channels(group=16)])
SIGMA48 = torch.tensor([0, 2, 3, 1])


def swizzle(img, axis, key):
    """LDS bank swizzle: gathers the logical image so that physical piece p of row r holds logical piece p ^ key(r).  `axis` is the
    piece axis, the axis before it the row axis; key maps the tensor of row numbers to the tensor of their XOR keys."""
    rows, pieces = img.shape[axis - 1], img.shape[axis]
    src = torch.arange(pieces)[None, :] ^ key(torch.arange(rows))[:, None]
    shape = [1] * img.dim()
    shape[axis - 1], shape[axis] = rows, pieces
    return torch.gather(img, axis, src.reshape(shape).expand(img.shape))


def streamed_image(w_ohwi, bn, device):
    """The streamed 3x3 kernels' weight image (layout: include/pam.h): [cout / bn][cin / 32][9 taps][bn rows][4 pieces][8] -- the rows of
    a slab by row_channels (a lane's accumulators are bn / 4 contiguous output channels), physical 16-byte piece p of row r = the
    chunk's input channels 8*(p ^ ((r >> 1) & 2)) .. + 7."""
    cout, _, _, cin = w_ohwi.shape
    w5 = w_ohwi.reshape(cout // bn, bn, 9, cin // 32, 32)[:, row_channels(group=bn)]            # [slab][row][tap][chunk][c]
    t = w5.permute(0, 3, 2, 1, 4).reshape(cout // bn, cin // 32, 9, bn, 4, 8)                   # [slab][chunk][tap][row][piece][8]
    return bf16_on(swizzle(t, axis=4, key=lambda r: (r >> 1) & 2), device)


def pointwise64_image(w_rows_by_k):
    """float32 LDS image of a pointwise convolution with 64 input channels for the kernels of csrc/pam_pw.hip (layouts: include/pam.h):
    w_rows_by_k [cout][64], cout a multiple of 64 -> [cout rows][8 pieces][8], rows in groups of 64 by row_channels, physical piece p
    of row r = input channels 8*(p ^ ((r >> 1) & 7)) .. + 7."""
    rows = w_rows_by_k.shape[0]
    w = w_rows_by_k[row_channels(group=64, groups=rows // 64)].reshape(rows, 8, 8)
    return swizzle(w, axis=1, key=lambda r: (r >> 1) & 7)


def kstep48_image(w_rows_by_k):
    """float32 k-step image of 3x3 convolutions with 48 input channels (k_bblock2_48, k_down48; layout: include/pam.h): w_rows_by_k
    [cout][K = (tap, cin) = 432], cout a multiple of 48 -> per 48-channel slab [14 k-steps of 32, zero tail][48 rows][4 pieces][8], rows
    by ROWS48, physical piece p of row r = logical piece p ^ sigma[(r % 16) >> 2], sigma = (0, 2, 3, 1)."""
    cout = w_rows_by_k.shape[0]
    wk = torch.zeros((cout, 14 * 32), dtype=torch.float32)
    wk[:, :432] = w_rows_by_k
    wk = wk.reshape(cout // 48, 48, 14, 4, 8)[:, ROWS48].permute(0, 2, 1, 3, 4)                 # [slab][k-step][row][piece][8]
    return swizzle(wk, axis=3, key=lambda r: SIGMA48[(r % 16) >> 2])


class PackedConv(object):
    def __init__(self, conv, device, pad_cin_to=None, pad_cout_to=None):
        """Zero-padding input channels (pad_cin_to) or output channels (pad_cout_to: zero filters, zero bias) leaves the real
        channels unchanged; the detector uses it for Darknet's 3-, 32- and 255-channel layers."""
        w = conv.weight.detach().float()
        b = bias_of(conv)
        cout, cin, kh, kw = w.shape
        if pad_cin_to is not None and cin < pad_cin_to:
            w = torch.cat([w, torch.zeros(cout, pad_cin_to - cin, kh, kw)], dim=1)
            cin = pad_cin_to
        if pad_cout_to is not None and cout < pad_cout_to:
            w = torch.cat([w, torch.zeros(pad_cout_to - cout, cin, kh, kw)], dim=0)
            b = torch.cat([b, torch.zeros(pad_cout_to - cout)])
            cout = pad_cout_to
        stem = cin == 8 and cout in (32, 64) and kh == 3 and kw == 3 and conv.stride[0] in (1, 2) and conv.padding[0] == 1
        # widths that are multiples of 32 only (HRNet-W32: 32, 224): the implicit GEMM with 32-channel slabs, k_conv3x3<32 | 256, 2>
        assert cin % 8 == 0 and (cout % 48 == 0 or cout % 64 == 0 or cout % 32 == 0 or stem), (cin, cout)
        ktot = kh * kw * cin
        kpad = (ktot + 63) // 64 * 64
        wp = torch.zeros((cout, kpad), dtype=torch.float32)
        wp[:, :ktot] = w.permute(0, 2, 3, 1).reshape(cout, ktot)          # k = (ky, kx, cin), cin fastest
        self.w = bf16_on(wp, device)
        self.bias = b.to(device).contiguous()
        self.cin, self.cout, self.kh, self.kw = cin, cout, kh, kw
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        # per-chunk LDS images for k_conv3x3, built lazily per slab width (the kernel picks the slab from the layer's H x W)
        self._w_ohwi = w.permute(0, 2, 3, 1).contiguous() if (kh == 3 and kw == 3 and self.stride == 1 and self.pad == 1 and
                                                              (cin in (48, 64, 96, 128, 192, 256, 384, 512) or
                                                               (cin == 32 and cout == 32))) else None
        self._images = {}
        self._device = device
        # stem convolution (8 -> 32 / 64 channels, 3x3, stride 1 / 2): the MFMA A fragments of k_conv_stem, [n-tile j][ky][lane][8]:
        # lane l holds, for row 16 j + (l & 15) of the one group of cout rows, the 8 input channels of tap (ky, kx = l >> 4)
        self._stem = None
        if stem:
            nt = cout // 16
            lanes = torch.arange(64)
            q, kx = lanes & 15, lanes >> 4
            chan = row_channels(group=cout).reshape(nt, 16)
            frag = torch.zeros((nt, 3, 64, 8), dtype=torch.float32)
            for j in range(nt):
                ch = chan[j][q]
                for ky in range(3):
                    sel = kx < 3
                    frag[j, ky, sel] = w[ch[sel], :, ky, kx[sel]]
            self._stem = bf16_on(frag, device)

    @staticmethod
    def merged(convs, device):
        """One convolution computing several same-shaped convolutions of the same input: weights / biases concatenated along
        the output channels, in the given order."""
        c0 = convs[0]
        assert all(c.kernel_size == c0.kernel_size and c.stride == c0.stride and c.padding == c0.padding and
                   c.in_channels == c0.in_channels for c in convs)
        m = nn.Conv2d(c0.in_channels, sum(c.out_channels for c in convs), c0.kernel_size, c0.stride, c0.padding, bias=True)
        with torch.no_grad():
            m.weight.copy_(torch.cat([c.weight.detach().float() for c in convs], 0))
            m.bias.copy_(torch.cat([bias_of(c) for c in convs]))
        return PackedConv(m, device)

    layout_lib = None           # tools/ab_conv_defs.py: a build variant whose layout functions decide the image (default: the library)

    def image(self, h, w, classic=False, c96_slab=0):
        """Weight image of this layer at input h x w for the rows-in-LDS kernels (layouts: include/pam.h): the classic per-chunk image
        [cout/BN][cin/CK][BN][pitch/2] (row = 9 taps x CK channels + pad), or -- where pam_conv3x3_layout() says so and the caller does
        not force the classic kernel -- the streamed kernel's image (streamed_image)."""
        if self._stem is not None:
            return self._stem
        if self._w_ohwi is None:
            return None
        from . import _lib
        lib = self.layout_lib or _lib.load()
        bn_s = 0 if classic else lib.pam_conv3x3_layout_ex(int(h), int(w), self.cin, self.cout, int(c96_slab))     # > 0: streamed kernel, with this slab width
        streamed = bn_s > 0
        bn = bn_s if streamed else lib.pam_conv3x3_slab(int(h), int(w), self.cin, self.cout)
        if self.cout % bn != 0:
            return None                                  # no whole number of slabs: the generic kernel takes this layer
        self.last_streamed = streamed                    # layout of the image this call returns (conv() states it to the library)
        self.last_c96 = bn if (streamed and self.cin == 96 and self.cout == 96) else 0
        img = self._images.get((bn, streamed))
        if img is None:
            if streamed:
                img = streamed_image(self._w_ohwi, bn, self._device)
            else:
                # k_conv3x3: the rows of a slab by row_channels (16-byte epilogue accesses), no swizzle (the pitch pads the banks)
                cin, cout = self.cin, self.cout
                ck = 48 if cin == 48 else (64 if cin >= 192 else 32)
                pitch = {48: 864, 32: 608, 64: 1184}[ck] // 2
                w5 = self._w_ohwi.reshape(cout // bn, bn, 9, cin // ck, ck)[:, row_channels(group=bn)]     # [slab][co][tap][chunk][c]
                t = torch.zeros((cout // bn, cin // ck, bn, pitch), dtype=torch.float32)
                t[:, :, :, :9 * ck] = w5.permute(0, 3, 1, 2, 4).reshape(cout // bn, cin // ck, bn, 9 * ck)
                img = bf16_on(t, self._device)
            self._images[(bn, streamed)] = img
        return img


def down48_image(op):
    """Weight image of a 3x3 stride-2 convolution with 48 input channels for ``pam_conv3x3s2_c48_nhwc_bf16`` (csrc/pam_down.hip; layout:
    include/pam.h): per 48-channel slab of the output one convolution of PackedBlock's C = 48 image (kstep48_image)."""
    assert op.cin == 48 and op.kh == 3 and op.kw == 3 and op.cout % 48 == 0
    img = getattr(op, '_down48', None)
    if img is None:
        img = op._down48 = bf16_on(kstep48_image(op.w[:, :432].float().cpu()), op._device)    # op.w: [cout][k = tap * 48 + cin]
        assert img.numel() * 2 == op.cout // 48 * 43008
    return img


class PackedUp(object):
    """The 1x1 convolutions into ONE output of an HR module's fuse layer, packed for ``pam_fuse_sum_nhwc_bf16`` (csrc/pam_fuse.hip):
    per coarser source branch the weights as MFMA A fragments [C / 16][Cs / 32][64 lanes][8] (lane l of fragment (j, ks) holds
    W[16 j + (l & 15)][32 ks + 8 (l >> 4) .. + 7]) and the float32 bias."""

    def __init__(self, convs, shifts, device):
        self.c = convs[0].weight.shape[0]
        self.shifts, self.chans, self.wimg, self.bias = list(shifts), [], [], []
        for cv in convs:
            c, cs = cv.weight.shape[0], cv.weight.shape[1]
            assert c == self.c and cv.weight.shape[2:] == (1, 1) and cs % 32 == 0 and c % 16 == 0
            w = cv.weight.detach().float().reshape(c // 16, 16, cs // 32, 4, 8).permute(0, 2, 3, 1, 4)     # [j][ks][g][q][8]
            self.wimg.append(bf16_on(w.reshape(c // 16, cs // 32, 64, 8), device))
            self.bias.append(bias_of(cv).to(device).contiguous())
            self.chans.append(cs)
        n = len(convs)
        self.c_w = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in self.wimg])
        self.c_b = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in self.bias])
        self.c_sh = (C.c_int32 * n)(*self.shifts)
        self.c_ch = (C.c_int32 * n)(*self.chans)


class PackedBlock(object):
    """One BasicBlock (conv3x3 -> ReLU -> conv3x3 -> + x -> ReLU) of the 32-, 48- or 96-channel branch packed for
    ``pam_basic_block2_nhwc_bf16`` (csrc/pam_block2.hip; layouts: include/pam.h): ONE buffer ``wpack`` =
    [float32 bias of conv1, conv2, padded to 1 KiB][k-step weight images of conv1][... of conv2]."""

    def __init__(self, conv1, conv2, device):
        c = conv1.weight.shape[0]
        assert c in (32, 48, 96) and conv1.weight.shape == (c, c, 3, 3) and conv2.weight.shape == (c, c, 3, 3)
        head = torch.zeros(256, dtype=torch.float32)
        head[:2 * c] = torch.cat([bias_of(conv1), bias_of(conv2)])
        ohwi = [cv.weight.detach().float().permute(0, 2, 3, 1) for cv in (conv1, conv2)]           # [cout][ky][kx][cin]
        if c == 32:
            # k_bblock2_32: K = (tap, cin), 9 k-steps of 32 (one per tap); a k-step image = [32 rows][4 pieces][8], one group of rows (a
            # lane ends with channels 8 g .. 8 g + 7: one 16-byte piece of a pixel), pieces swizzled by (R >> 2) & 3
            imgs = [swizzle(w[row_channels(group=32)].reshape(c, 9, 4, 8).permute(1, 0, 2, 3), axis=2, key=lambda r: (r >> 2) & 3) for w in ohwi]
            ksteps = 9
        elif c == 48:
            # k_bblock2_48: K = (tap, cin) flattened, 14 k-steps of 32 (zero tail): kstep48_image
            imgs = [kstep48_image(w.reshape(c, 9 * c))[0] for w in ohwi]
            ksteps = 14
        else:
            # k_bblock2_96: k-step images [96 rows][4 pieces][8] in the order (conv, chunk of 32 input channels, tap); one group of rows (a
            # lane ends with 24 contiguous channels), physical piece p of row r holds the chunk's input channels 8 * (p ^ ((r >> 1) & 2)) .. + 7
            imgs = [swizzle(w[row_channels(group=96)].reshape(c, 9, 3, 4, 8).permute(2, 1, 0, 3, 4), axis=3, key=lambda r: (r >> 1) & 2)
                    for w in ohwi]                                                                 # [chunk][tap][row][piece][8]
            ksteps = 27
        self.wpack = torch.cat([head.view(torch.uint8), torch.stack(imgs).to(torch.bfloat16).reshape(-1).view(torch.uint8)]).to(device).contiguous()
        assert self.wpack.numel() == 1024 + 2 * ksteps * c * 64
        self.c = c


class PackedTail(object):
    """The pointwise tail of a layer1 Bottleneck packed for ``pam_bottleneck_tail_nhwc_bf16`` (csrc/pam_pw.hip; layouts: include/pam.h):
    conv3 (64 -> 256) [+ the first block's 1x1 downsample as a second K chunk] and, optionally, the NEXT block's conv1 (256 -> 64)."""

    def __init__(self, conv3, down, conv1_next, device):
        assert conv3.weight.shape == (256, 64, 1, 1) and (down is None or down.weight.shape == (256, 64, 1, 1))
        assert conv1_next is None or conv1_next.weight.shape == (64, 256, 1, 1)
        srcs = [conv3] + ([down] if down is not None else [])
        self.w3 = bf16_on(torch.stack([pointwise64_image(cv.weight.detach().float().reshape(256, 64)) for cv in srcs]), device)
        self.b3 = (bias_of(conv3) + (bias_of(down) if down is not None else 0)).to(device).contiguous()
        self.S = len(srcs)
        self.w1 = self.b1 = None
        if conv1_next is not None:
            # w1 [4 K chunks of 64][64 rows][8 pieces][8]: the K order of a chunk is the lane order of conv3's accumulators -- logical
            # piece q = input channels 64 sl + 16 (q & 3) + 8 (q >> 2) .. + 7; rows and swizzle as pointwise64_image
            w = conv1_next.weight.detach().float().reshape(64, 256)[row_channels(group=64)]        # [row][input channel]
            w = w.reshape(64, 4, 4, 2, 8).permute(1, 0, 3, 2, 4).reshape(4, 64, 8, 8)               # [chunk][row][q = 4 (q >> 2) + (q & 3)][8]
            self.w1 = bf16_on(swizzle(w, axis=2, key=lambda r: (r >> 1) & 7), device)
            self.b1 = bias_of(conv1_next).to(device).contiguous()


class PackedPointwise64(object):
    """A 64 -> 64 1x1 convolution (+ ReLU) packed for ``pam_pointwise64_relu_nhwc_bf16`` (csrc/pam_pw.hip, k_pw1)."""

    def __init__(self, conv, device):
        assert conv.weight.shape == (64, 64, 1, 1)
        self.w = bf16_on(pointwise64_image(conv.weight.detach().float().reshape(64, 64)), device)
        self.b = bias_of(conv).to(device).contiguous()


def conv64_image(conv, device):
    """[9 taps][64 rows][64 K] bf16 LDS image of a 64 -> 64 3x3 convolution for the fused stem / Bottleneck kernels (layout: include/pam.h):
    two groups of 32 rows -- a lane then ends with channels 32 h + 8 g .. + 7, the natural K order of the pointwise product that consumes
    its accumulators --, 16-byte pieces swizzled by (row >> 1) & 7."""
    assert conv.weight.shape == (64, 64, 3, 3)
    w = conv.weight.detach().float()[row_channels(group=32, groups=2)]                          # [row][cin][ky][kx]
    img = swizzle(w.permute(2, 3, 0, 1).reshape(9, 64, 8, 8), axis=2, key=lambda r: (r >> 1) & 7)
    return bf16_on(img.reshape(9, 64, 64), device)


class PackedBneck(object):
    """A layer1 Bottleneck from its 3x3 convolution on, packed for ``pam_bottleneck_fused_nhwc_bf16`` (csrc/pam_bneck.hip): the 3x3's LDS
    image + the pointwise tail's images (PackedTail with one K source)."""

    def __init__(self, conv2, tail, device):
        assert conv2.stride[0] == 1 and conv2.padding[0] == 1
        self.tail = tail
        self.w2 = conv64_image(conv2, device)
        self.b2 = bias_of(conv2).to(device).contiguous()


class PackedStem(object):
    """HRNet's stem (conv1 8 -> 64 s2, conv2 64 -> 64 s2) and layer1[0].conv1 (64 -> 64 1x1) packed for ``pam_stem_fused_nhwc_bf16``
    (csrc/pam_stem.hip; layouts: include/pam.h): conv1 and the pointwise keep the images of their own kernels, conv2 gets the
    [9 taps][64 rows][64 K] LDS image."""

    def __init__(self, conv1_packed, conv2, pw_packed, device):
        assert conv1_packed._stem is not None and conv1_packed.cout == 64 and conv1_packed.stride == 2
        assert conv2.weight.shape == (64, 64, 3, 3) and conv2.stride[0] == 2 and conv2.padding[0] == 1
        self.c1, self.pw = conv1_packed, pw_packed
        self.w2 = conv64_image(conv2, device)
        self.b2 = bias_of(conv2).to(device).contiguous()


class PackedResNetStem(object):
    """PoseResNet's conv1 (3 -> 64, 7x7 stride 2, BN folded) packed for ``pam_resnet_stem_nhwc_bf16`` (csrc/pam_resnet.hip; layout:
    include/pam.h, poseresnet.stem_fragments); the max-pool after it has no weights."""

    def __init__(self, conv, device):
        from .poseresnet import stem_fragments
        self.frag = bf16_on(stem_fragments(conv), device)
        self.bias = bias_of(conv).to(device).contiguous()


class PackedDeconv(object):
    """A 4x4 stride-2 transposed convolution (BN folded) packed for ``pam_deconv4x4s2_nhwc_bf16``: the per-parity weight image of
    poseresnet.deconv_image (layout: include/pam.h)."""

    def __init__(self, deconv, device):
        from .poseresnet import deconv_image
        w = deconv.weight.detach().float()
        assert tuple(w.shape[2:]) == (4, 4) and deconv.stride == (2, 2) and deconv.padding == (1, 1) and deconv.output_padding == (0, 0)
        self.cin, self.cout = int(w.shape[0]), int(w.shape[1])
        self.w = bf16_on(deconv_image(w), device)
        self.bias = bias_of(deconv, n=self.cout).to(device).contiguous()


# -- the token kernels' linear layers (csrc/pam_vit.hip) ---------------------------------------------------------------------------------
def linear_image(w):
    """(N, K) float32 -> the flat image of pam_vit_linear_bf16 (layout: include/pam.h): [N / 64 slabs s][K / 32 k-steps c][4 n-tiles j]
    [64 lanes][8]; lane l holds output channel 64 s + 16 ((l & 15) >> 2) + 4 j + (l & 3) and input channels 32 c + 8 (l >> 4) .. + 7."""
    n, k = w.shape
    assert n % 64 == 0 and k % 64 == 0, (n, k)
    w7 = w.reshape(n // 64, 4, 4, 4, k // 32, 4, 8)                        # [s][a = (l & 15) >> 2][j][b = l & 3][c][g = l >> 4][8]
    return w7.permute(0, 4, 2, 5, 1, 3, 6).reshape(-1)                     # [s][c][j][g][a][b][8]: lane = 16 g + 4 a + b


def linear_unimage(img, n, k):
    """The inverse of ``linear_image``: the flat image -> the (N, K) matrix (the packing round trip of the tests)."""
    t = img.reshape(n // 64, k // 32, 4, 4, 4, 4, 8)                        # [s][c][j][g][a][b][8]
    return t.permute(0, 4, 2, 5, 1, 3, 6).reshape(n, k)


class PackedLinear(object):
    """A linear layer y = x W^T + b (weight (N, K), N and K multiples of 64) packed for ``pam_vit_linear_bf16``; with K = 2048 rows in
    the order (ky, kx, 8 channels) the same image is the patch embedding's (``pam_vit_patch_embed_bf16``; vitpose.patch_matrix)."""

    def __init__(self, weight, bias, device):
        w = weight.detach().float()
        self.n, self.k = int(w.shape[0]), int(w.shape[1])
        self.w = bf16_on(linear_image(w), device)
        self.bias = (bias.detach().float() if bias is not None else torch.zeros(self.n)).to(device).contiguous()
