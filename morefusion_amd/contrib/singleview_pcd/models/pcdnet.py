"""Inference of the point-cloud baseline network on the hand-written path (DESIGN.md "Point-cloud baseline network").

Rows are points, m = b * P + p.  The point-wise kernels are csrc/pcdnet.hip (stem, pool, bias + ReLU + split), the
GEMM layers run on ``mf_linear_split_fwd`` (split-bf16 MFMA) and, for the per-object part of the heads' first layer,
on ``mf_linear_fwd`` (fp32 MFMA); the pose epilogue is ``mf_pose_epilogue`` with pts = p - center, origin = center,
pitch = 1, which is the reference's ((p - c) + c) + t in fp32.

The fold: 1024 of the 1408 input channels of the heads' first layer are the pooled vector repeated over the points,
so ``W[:, 384:] @ pooled[b] + bias`` is a per-object bias (``gbias`` [B, 1920]) and the per-point GEMM keeps K = 384.

Split layouts (bf16; the engine reads the lo plane Kp columns behind the hi plane of the same row):
  f1   [M, 256]   rgb hi 64 | rgb lo 64 | pcd hi 64 | pcd lo 64          conv2_rgb / conv2_pcd read one half each
  xs   [M, 768]   hi 384 | lo 384 of (feat1 rgb | feat1 pcd | feat2 rgb | feat2 pcd)   conv3 and heads layer 1 read it
  h3   [M, 1024]  hi 512 | lo 512                                         conv4 reads it
  h1   [M, 3840]  per head hi 640 | lo 640                                heads layer 2
  h2   [M, 1536]  per head hi 256 | lo 256;  h3h [M, 768] per head hi 128 | lo 128
conv3 reads xs with Kp = 384 and zero weights over feat1's 128 channels (written by the stem before conv2 runs), so
feat2 is written once, where both of its readers find it.
"""
import ctypes

import torch

from .... import _lib

HEADS = ("rot", "trans", "conf")
N_BUFFERS = 12


class PcdNetKernels:
    """Weight packs, the workspace and the launch sequence; one instance per Model."""

    def __init__(self, model):
        self.m = model
        self._packs = {}
        self._ws = {}

    # ---- cached weight packs (re-packed when a parameter changes in place or is re-assigned) ----
    def _pack(self, name, tensors, build):
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        hit = self._packs.get(name)
        if hit is None or hit[0] != key:
            hit = (key, build())
            self._packs[name] = hit
        return hit[1]

    @staticmethod
    def _split_pack(w, Kp):
        """fp32 [N, K] -> the engine's bf16 [N, 3 Kp] = (w_hi | w_hi | w_lo), zero columns up to Kp."""
        w = w.contiguous()
        N, K = w.shape
        wp = torch.empty((N, 3 * Kp), dtype=torch.bfloat16, device=w.device)
        _lib.check(_lib.lib().mf_linear_split_pack(w.data_ptr(), 0, K, N, K, N, Kp, 1, wp.data_ptr(), _lib.stream_ptr()),
                   "mf_linear_split_pack")
        return wp

    def _w(self, conv):
        return conv.weight.detach().float().squeeze(-1)

    def packs(self):
        m, e = self.m, self.m.posenet_extractor
        convs = [e.conv1_rgb, e.conv1_pcd, e.conv2_rgb, e.conv2_pcd, e.conv3, e.conv4] + [
            getattr(m, f"conv{i}_{k}") for i in (1, 2, 3, 4) for k in HEADS]

        def build():
            nf = m._n_fg_class
            np4 = -(-(4 * nf) // 8) * 8
            p = {"np4": np4}
            p["stem"] = (self._w(e.conv1_rgb).contiguous(), e.conv1_rgb.bias.detach().float().contiguous(),
                         self._w(e.conv1_pcd).contiguous(), e.conv1_pcd.bias.detach().float().contiguous())
            for name, conv in (("conv2_rgb", e.conv2_rgb), ("conv2_pcd", e.conv2_pcd), ("conv4", e.conv4)):
                p[name] = (self._split_pack(self._w(conv), conv.in_channels), conv.bias.detach().float().contiguous())
            w3 = self._w(e.conv3)
            w3 = torch.cat([torch.zeros((w3.shape[0], 128), dtype=w3.dtype, device=w3.device), w3], dim=1)
            p["conv3"] = (self._split_pack(w3, 384), e.conv3.bias.detach().float().contiguous())
            w1 = torch.cat([self._w(getattr(m, f"conv1_{k}")) for k in HEADS])            # [1920, 1408]
            p["heads1_point"] = self._split_pack(w1[:, :384], 384)
            p["heads1_global"] = (w1[:, 384:].contiguous(),
                                  torch.cat([getattr(m, f"conv1_{k}").bias.detach().float() for k in HEADS]).contiguous())
            for i, Kp in ((2, 640), (3, 256)):
                p[f"heads{i}"] = [(self._split_pack(self._w(getattr(m, f"conv{i}_{k}")), Kp),
                                   getattr(m, f"conv{i}_{k}").bias.detach().float().contiguous()) for k in HEADS]
            p["heads4"] = []
            for k in HEADS:  # N = n_fg * {4, 3, 1} -> np4 rows (zero weights and bias beyond N: the engine needs N % 8 == 0)
                c = getattr(m, f"conv4_{k}")
                w = torch.zeros((np4, 128), dtype=torch.float32, device=c.weight.device)
                b = torch.zeros((np4,), dtype=torch.float32, device=w.device)
                w[:c.out_channels] = self._w(c)
                b[:c.out_channels] = c.bias.detach().float()
                p["heads4"].append((self._split_pack(w, 128), b))
            return p
        return self._pack("all", [t for c in convs for t in (c.weight, c.bias)], build)

    def workspace(self, B, P, device):
        """The activation buffers of one (B, P) as views of ONE allocation (mf_pcdnet_workspace_offsets), and the
        split-K workspace of the GEMMs."""
        key = (B, P, str(device))
        hit = self._ws.get(key)
        if hit is not None:
            return hit
        L, nf = _lib.lib(), self.m._n_fg_class
        off = (ctypes.c_int64 * (N_BUFFERS + 1))()
        if L.mf_pcdnet_workspace_offsets(B, P, nf, ctypes.addressof(off)) != N_BUFFERS:
            raise ValueError(f"pcdnet: no workspace for B = {B}, P = {P}, n_fg = {nf}")
        assert off[N_BUFFERS] == L.mf_pcdnet_workspace_bytes(B, P, nf)
        raw = torch.empty((off[N_BUFFERS],), dtype=torch.uint8, device=device)
        M, np4 = B * P, -(-(4 * nf) // 8) * 8
        f32, b16 = torch.float32, torch.bfloat16
        spec = (("pts", f32, (M, 3)), ("f1", b16, (M, 256)), ("xs", b16, (M, 768)), ("h3", b16, (M, 1024)),
                ("h4", f32, (M, 1024)), ("pooled", f32, (B, 1024)), ("gbias", f32, (B, 1920)), ("y", f32, (M, 1920)),
                ("h1", b16, (M, 3840)), ("h2", b16, (M, 1536)), ("h3h", b16, (M, 768)), ("o", f32, (M, 3 * np4)))
        bufs = {"raw": raw}
        for (name, dt, shape), o in zip(spec, off):
            n = shape[0] * shape[1] * (4 if dt == f32 else 2)
            bufs[name] = raw[o:o + n].view(dt).view(shape)
        need = max(L.mf_linear_split_workspace_bytes(M, N, Kp) for N, Kp in
                   ((128, 64), (512, 384), (1024, 512), (1920, 384), (256, 640), (128, 256), (np4, 128)))
        bufs["splitk"] = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
        self._ws[key] = bufs
        return bufs

    def _gemm(self, ws, a, lda, wp, bias, relu, M, N, Kp, out32=None, ldo32=0, outs=None, ldos=0, los=0):
        L = _lib.lib()
        nbytes = L.mf_linear_split_workspace_bytes(M, N, Kp)
        _lib.check(L.mf_linear_split_fwd(a.data_ptr(), lda, wp.data_ptr(), _lib.ptr(bias), int(relu), _lib.ptr(out32),
                                         ldo32, _lib.ptr(outs), ldos, los, ws["splitk"].data_ptr(), nbytes, M, N, Kp,
                                         _lib.stream_ptr()), "mf_linear_split_fwd")

    # ---- stages (each usable alone: tests and tools/time_pcd_predict.py) ------------------------------
    def stem(self, ws, p, rows, pcd, pix, center, B, P):
        w_rgb, b_rgb, w_pcd, b_pcd = p["stem"]
        HW = pcd.shape[1] * pcd.shape[2]
        _lib.check(_lib.lib().mf_pcdnet_stem(
            rows.data_ptr(), pcd.data_ptr(), pix.data_ptr(), _lib.ptr(center), w_rgb.data_ptr(), b_rgb.data_ptr(),
            w_pcd.data_ptr(), b_pcd.data_ptr(), B, P, HW, ws["pts"].data_ptr(), ws["f1"].data_ptr(), 256,
            ws["xs"].data_ptr(), 768, 384, _lib.stream_ptr()), "mf_pcdnet_stem")

    def extractor(self, ws, p, M):
        """conv2 (two launches), conv3, conv4 on the split rows -> h4 fp32 [M, 1024]."""
        f1, xs = ws["f1"], ws["xs"]
        self._gemm(ws, f1, 256, *p["conv2_rgb"], True, M, 128, 64, outs=xs[:, 128:], ldos=768, los=384)
        self._gemm(ws, f1[:, 128:], 256, *p["conv2_pcd"], True, M, 128, 64, outs=xs[:, 256:], ldos=768, los=384)
        self._gemm(ws, xs, 768, *p["conv3"], True, M, 512, 384, outs=ws["h3"], ldos=1024, los=512)
        self._gemm(ws, ws["h3"], 1024, *p["conv4"], True, M, 1024, 512, out32=ws["h4"], ldo32=1024)

    def pool(self, ws, B, P):
        _lib.check(_lib.lib().mf_pcdnet_pool(ws["h4"].data_ptr(), 1024, B, P, 1024, ws["pooled"].data_ptr(),
                                             _lib.stream_ptr()), "mf_pcdnet_pool")

    def heads1(self, ws, p, B, P):
        """Heads layer 1 folded: gbias = W[:, 384:] pooled + b (one M = B GEMM), y = xs W[:, :384]^T (per point),
        h1 = relu(y + gbias[m / P]) in split form."""
        L, M = _lib.lib(), B * P
        wg, bg = p["heads1_global"]
        _lib.check(L.mf_linear_fwd(ws["pooled"].data_ptr(), 0, 1024, wg.data_ptr(), 0, 1024, bg.data_ptr(), 0,
                                   ws["gbias"].data_ptr(), 0, 1920, B, 1920, 1920, 1024, 1, 0, _lib.stream_ptr()),
                   "mf_linear_fwd")
        self._gemm(ws, ws["xs"], 768, p["heads1_point"], None, False, M, 1920, 384, out32=ws["y"], ldo32=1920)
        _lib.check(L.mf_pcdnet_bias_relu_split(ws["y"].data_ptr(), 1920, ws["gbias"].data_ptr(), B, P, 1920, 640,
                                               ws["h1"].data_ptr(), 3840, _lib.stream_ptr()),
                   "mf_pcdnet_bias_relu_split")

    def heads234(self, ws, p, M):
        np4 = p["np4"]
        for g in range(3):
            self._gemm(ws, ws["h1"][:, 1280 * g:], 3840, *p["heads2"][g], True, M, 256, 640,
                       outs=ws["h2"][:, 512 * g:], ldos=1536, los=256)
        for g in range(3):
            self._gemm(ws, ws["h2"][:, 512 * g:], 1536, *p["heads3"][g], True, M, 128, 256,
                       outs=ws["h3h"][:, 256 * g:], ldos=768, los=128)
        for g in range(3):
            self._gemm(ws, ws["h3h"][:, 256 * g:], 768, *p["heads4"][g], False, M, np4, 128,
                       out32=ws["o"][:, np4 * g:], ldo32=3 * np4)

    def epilogue(self, ws, p, class_id, center, B, P):
        dev, np4 = ws["o"].device, p["np4"]
        rot = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
        trans = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
        conf = torch.empty((B, P), dtype=torch.float32, device=dev)
        cid = class_id.to(device=dev, dtype=torch.int64).contiguous()
        origin = center if center is not None else torch.zeros((B, 3), dtype=torch.float32, device=dev)
        one = torch.ones((B,), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mf_pose_epilogue(ws["o"].data_ptr(), 3 * np4, np4, cid.data_ptr(), ws["pts"].data_ptr(),
                                               origin.data_ptr(), one.data_ptr(), B, P, self.m._n_fg_class,
                                               rot.data_ptr(), trans.data_ptr(), conf.data_ptr(), _lib.stream_ptr()),
                   "mf_pose_epilogue")
        return rot, trans, conf

    def pose(self, class_id, rows, pcd, pix, center):
        """rows fp32 [B*P, 32] (the PSPNet tail's rows), pcd fp32 [B,H,W,3], pix int64 [B,P], center fp32 [B,3] or
        None -> (rot [B,P,4], trans [B,P,3], conf [B,P]) of each object's class."""
        B, P = pix.shape
        _lib.require_gpu(rows, pcd, pix)
        rows, pcd = _lib.f32c(rows), _lib.f32c(pcd)
        pix = pix.reshape(-1).to(torch.int64).contiguous()
        center = None if center is None else _lib.f32c(center)
        p, ws = self.packs(), self.workspace(B, P, rows.device)
        self.stem(ws, p, rows, pcd, pix, center, B, P)
        self.extractor(ws, p, B * P)
        self.pool(ws, B, P)
        self.heads1(ws, p, B, P)
        self.heads234(ws, p, B * P)
        return self.epilogue(ws, p, class_id, center, B, P)
