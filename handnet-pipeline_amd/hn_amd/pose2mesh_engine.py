"""Pose2Mesh lifter on MI355X: 2-D hand joints -> 3-D joints (MLP) -> mesh vertices (Chebyshev graph convs).

Arithmetic follows pose2mesh/lib/models/pose2mesh_net.py:17-24, posenet.py:27-41,78-88 (eval) and
meshnet.py:79-117 ('mano' configuration, K = 3) of the reference:
  Linear / Linear+BatchNorm1d(+ReLU)      -> hn_conv2d_nhwc_f16x3_ws as a 1x1 convolution over [batch][vertex]
                                             rows (split-fp16 operands, fp32-grade; BatchNorm folded in fp64;
                                             long-k layers such as the 4096x4096 MLP run split-K)
  pre-activation BatchNorm+ReLU (posenet) -> hn_affine_split_f32 (the same pass that feeds GroupNorm'd towers)
  Chebyshev recursion x1 = L x0, x2 = 2 L x1 - x0 and the (fin, k) concat -> hn_spmm_csr_f32 +
                                             hn_cheby3_basis_split, which writes the conv's S32 operand directly
                                             (k-major channel order; the Linear's columns are permuted to match)
  block residual (feature-axis linear interpolation + add) and nearest x2 vertex up-sampling
                                          -> hn_feat_interp_add_f32
Everything stays on the device.  Graph Laplacians are host-side preprocessing (graph_utils.build_coarse_graphs),
passed in as scipy / torch sparse matrices, finest level first, joint graph last.

Launch structure (round 6; the forward is launch-bound at the live caller's batch): `fused=True` (default) runs the forward as
23 launches instead of 76 at 1..4 samples (26 above) --
  PoseNet   1..4 samples: six matrix-vector launches (hn_linear_rows_f16x3: pre-activation BatchNorm + ReLU applied while the
            activations are staged, batch_norm2 FOLDED into the Linear in front of it, residual in the epilogue)     = 6
            larger batches: hn_pad_split_rows_f32 (the input operand), then per stage the pre-activation BatchNorm + ReLU +
            split pass, Linear 1 (+ folded batch_norm2) + ReLU + split, Linear 2 + residual on the convolution kernel = 9
  glue      hn_lifter_combine_f32 (pose_combine, zero padded to the first graph convolution's 8 input features)       = 1
  mesh net  ONE launch per graph convolution (hn_graph_conv_cheby3_f16x3: basis gather -> MFMA -> bias / ReLU -> the
            block's residual + vertex up-sampling in the epilogue of its last layer; the layer in front of `fc` writes
            fc's S32 operand), + fc                                                                                  = 16
`fused=False` keeps the layer-by-layer structure of rounds 2-5 (spmm, basis, 1x1 convolution, residual pass): the reference
form of the tests and of the same-box A/B.
"""
from __future__ import annotations

import torch

from . import ops
from .weights import ConvW, split_f16x3

CL_F = [(5, 32, 64, 64), (64, 128, 256), (256, 256, 256), (256, 256, 256), (256, 256, 256), (256, 128, 128),
        (128, 64, 3)]   # meshnet.py:22-27
CL_K = 3
BN_EPS = 1e-5


def _pad32(c):
    return (c + 31) // 32 * 32


def _dense(weight, bias, device, cin_pad=None) -> ConvW:
    """[Fout, Fin] fp64 -> 1x1 conv weights with Cin padded to a multiple of 32."""
    fout, fin = weight.shape
    cpad = _pad32(fin) if cin_pad is None else cin_pad
    w = torch.zeros((fout, 1, 1, cpad), dtype=torch.float32)
    w[:, 0, 0, :fin] = weight.float()
    return ConvW(w.contiguous(), None if bias is None else bias.float().contiguous(), 1, 0, 1, split_f16x3(w)).to(device)


class Pose2MeshEngine:
    def __init__(self, state_dict, graph_L, num_joint: int = 21, device="cuda", fused: bool = True):
        sd = {k: v.detach().double().cpu() for k, v in state_dict.items() if v.dtype.is_floating_point}
        dev = torch.device(device)
        self.device, self.num_joint, self.fused = dev, num_joint, bool(fused)
        self._graphs = {}
        self._bn_rows = {}
        graph_L = [self._as_scipy(L) for L in graph_L]
        levels = [ops.csr_graph(L, dev) for L in graph_L]
        levels2 = [ops.cheby2_graph(L, dev) for L in graph_L]         # 2 L L - I per level (the fused graph convolution)
        del levels[-2]                                   # meshnet.py:37
        del levels2[-2]
        self.graphs, self.graphs2 = levels, levels2
        if levels[-1].v != num_joint:
            raise ValueError("the last graph must be the joint graph")
        p = "pose_lifter."
        self.p_w1 = _dense(sd[p + "w1.weight"], sd[p + "w1.bias"], dev)
        self.p_stages = []
        for st in range(2):
            q = f"{p}linear_stages.{st}."
            # batch_norm2 sits directly behind w1 (posenet.py:28-31): folded into its rows in fp64 for the fused structure
            s2 = sd[q + "batch_norm2.weight"] / torch.sqrt(sd[q + "batch_norm2.running_var"] + BN_EPS)
            t2 = sd[q + "batch_norm2.bias"] - sd[q + "batch_norm2.running_mean"] * s2
            self.p_stages.append({
                "bn1": self._bn_table(sd, q + "batch_norm1", dev), "w1": _dense(sd[q + "w1.weight"], sd[q + "w1.bias"], dev),
                "w1_bn2": _dense(sd[q + "w1.weight"] * s2.view(-1, 1), sd[q + "w1.bias"] * s2 + t2, dev),
                "bn2": self._bn_table(sd, q + "batch_norm2", dev), "w2": _dense(sd[q + "w2.weight"], sd[q + "w2.bias"], dev)})
        # the output Linear with its rows zero-padded to a multiple of 8 (63 -> 64): the convolution kernel's vectorised
        # epilogue, and with it split-K, needs Cout % 8 == 0 -- unsplit, this one launch walked 128 k tiles in a row (40 us of
        # the 0.37 ms forward at batch 1)
        w2, b2 = sd[p + "w2.weight"], sd[p + "w2.bias"]
        self.p_out = w2.shape[0]
        padr = (-w2.shape[0]) % 8
        if padr:
            w2 = torch.cat([w2, torch.zeros((padr, w2.shape[1]), dtype=w2.dtype)])
            b2 = torch.cat([b2, torch.zeros((padr,), dtype=b2.dtype)])
        self.p_w2 = _dense(w2, b2, dev)
        m = "pose2mesh."
        self.fc = _dense(sd[m + "fc.weight"], sd[m + "fc.bias"], dev)
        self.cl = []
        idx = 0
        for bi, chain in enumerate(CL_F):
            for li in range(len(chain) - 1):
                fin, fout = chain[li], chain[li + 1]
                fin_pad = (fin + 3) // 4 * 4 if fin % 4 else fin
                fin_pad = max(fin_pad, 8) if fin % 4 else fin_pad
                w = sd[f"{m}cl.{idx}.weight"].view(fout, fin, CL_K)          # reference column order (fin, k)
                b = sd[f"{m}cl.{idx}.bias"]
                last = bi == len(CL_F) - 1 and li == len(chain) - 2
                if not last:                                                  # fold BatchNorm1d (eval)
                    s = sd[f"{m}bn.{idx}.weight"] / torch.sqrt(sd[f"{m}bn.{idx}.running_var"] + BN_EPS)
                    w = w * s.view(-1, 1, 1)
                    b = (b - sd[f"{m}bn.{idx}.running_mean"]) * s + sd[f"{m}bn.{idx}.bias"]
                wk = torch.zeros((fout, CL_K, fin_pad), dtype=torch.float64)  # k-major, features zero-padded
                wk[:, :, :fin] = w.permute(0, 2, 1)
                cw = _dense(wk.reshape(fout, CL_K * fin_pad), b, dev)
                cw.w_frag = ops.fragment_order(cw.w16)          # (the fused graph convolution's contiguous fragment loads)
                self.cl.append((cw, fin_pad, not last))
                idx += 1

    # The one-launch graph convolution is a LATENCY design (16 rows per 1024-thread workgroup, every workgroup gathers its own
    # basis rows): it wins where the forward is launch-bound.  Larger batches are throughput-bound and run the mesh net
    # layer by layer (streaming spmm / basis passes + the tiled 1x1 convolution).
    FUSED_MAX_BATCH = 4

    @staticmethod
    def _as_scipy(L):
        if torch.is_tensor(L):
            import scipy.sparse as sp
            c = L.coalesce() if L.layout == torch.sparse_coo else L.to_sparse_coo().coalesce()
            idx = c.indices().cpu().numpy()
            return sp.csr_matrix((c.values().cpu().numpy(), (idx[0], idx[1])), shape=tuple(c.shape))
        return L.tocsr()

    def _rows(self, table, b):
        """a [C] BatchNorm table as the [b, C] rows hn_affine_split_f32 takes (built once per batch size)"""
        key = (table.data_ptr(), b)
        t = self._bn_rows.get(key)
        if t is None:
            with torch.inference_mode(False):
                t = self._bn_rows[key] = table.expand(b, -1).contiguous()
        return t

    @staticmethod
    def _bn_table(sd, name, dev):
        s = sd[name + ".weight"] / torch.sqrt(sd[name + ".running_var"] + BN_EPS)
        t = sd[name + ".bias"] - sd[name + ".running_mean"] * s
        return s.float().to(dev), t.float().to(dev)

    # -----------------------------------------------------------------------------------
    def _linear(self, x, cw: ConvW, relu=False, residual=None):
        """x: S32 [B,1,1,...] or fp32 [B,1,1,C] -> fp32 [B,1,1,Fout]"""
        return ops.conv2d_nhwc(x, cw.w, cw.bias, relu=relu, residual=residual, w16=cw.w16)

    def posenet(self, x2d):
        """[B, 2J] fp32 -> [B, 3J] (LinearModel.forward, eval)"""
        b = x2d.shape[0]
        if self.fused and b <= self.FUSED_MAX_BATCH:
            # 1..4 rows: every Linear is a matrix-vector product on the vector ALU (hn_linear_rows_f16x3: the 67 MB bank streamed
            # once, fp32 activations staged in LDS through the pre-activation BatchNorm + ReLU) -- 6 launches, no split passes
            y = ops.linear_rows(x2d.contiguous(), self.p_w1)
            for st in self.p_stages:
                z = ops.linear_rows(y, st["w1_bn2"], scale=st["bn1"][0], shift=st["bn1"][1], relu=True)
                y = ops.linear_rows(z, st["w2"], residual=y)
            return ops.linear_rows(y, self.p_w2)[:, : self.p_out]
        if self.fused:
            y = self._linear(ops.pad_split_rows(x2d.contiguous(), self.p_w1.cin), self.p_w1)
            last = len(self.p_stages) - 1
            for i, st in enumerate(self.p_stages):
                a = ops.to_split(y, self._rows(st["bn1"][0], b), self._rows(st["bn1"][1], b), relu=True)
                cw = st["w1_bn2"]
                z = ops.conv2d_nhwc(a, cw.w, cw.bias, relu=True, w16=cw.w16, out_split=True)
                cw = st["w2"]
                y = ops.conv2d_nhwc(z, cw.w, cw.bias, residual=y, w16=cw.w16, out_split=i == last)
            return self._linear(y, self.p_w2).reshape(b, -1)[:, : self.p_out]
        xin = torch.zeros((b, 1, 1, self.p_w1.cin), device=self.device, dtype=torch.float32)
        xin[:, 0, 0, : x2d.shape[1]] = x2d
        y = self._linear(xin, self.p_w1)
        for st in self.p_stages:
            s1, t1 = (t.expand(b, -1).contiguous() for t in st["bn1"])
            z = self._linear(ops.to_split(y, s1, t1, relu=True), st["w1"])
            s2, t2 = (t.expand(b, -1).contiguous() for t in st["bn2"])
            y = self._linear(ops.to_split(z, s2, t2, relu=True), st["w2"], residual=y)
        return self._linear(y, self.p_w2).reshape(b, -1)[:, : self.p_out]

    def _graph_conv(self, x, layer, g):
        cw, fin_pad, relu = layer
        b, v, f = x.shape
        if f != fin_pad:
            xp = torch.zeros((b, v, fin_pad), device=self.device, dtype=torch.float32)
            xp[..., :f] = x
            x = xp
        x = x.contiguous()
        basis = ops.cheby3_basis_split(g, x, ops.spmm_csr(g, x))
        return ops.conv2d_nhwc(basis, cw.w, cw.bias, relu=relu, w16=cw.w16).view(b, v, -1)

    def meshnet_fused(self, x, mesh_out=None):
        """[B, J, 8] (pose_combine, zero padded) -> [B, V0, 3]: one launch per graph convolution (+ fc); mesh_out: a
        preallocated fp32 [B, V0, 3] the last layer writes (the live step's copy buffer)"""
        b = x.shape[0]
        nblk = len(CL_F)
        li = 0
        for i in range(nblk):
            xin = x
            lv = -(i + 1) + (1 if i == nblk - 1 else 0)
            g, g2 = self.graphs[lv], self.graphs2[lv]
            nl = len(CL_F[i]) - 1
            for k in range(nl):
                cw, fin_pad, relu = self.cl[li]
                li += 1
                last = k == nl - 1
                if last and i == 0:                # the layer in front of fc writes fc's S32 operand ([B, 1, 1, V * F])
                    x = ops.graph_conv_cheby3(g, g2, x, cw, relu=relu, out_split=True)
                    x = self._linear(x.view(b, 1, 1, -1, 2, 32), self.fc).view(b, self.graphs[-2].v, CL_F[1][0])
                elif last and 0 < i < nblk - 1:    # block residual (+ nearest x2 vertex up-sampling) in the epilogue
                    x = ops.graph_conv_cheby3(g, g2, x, cw, relu=relu, xin=xin, up=2 if i < nblk - 2 else 1)
                else:
                    final = i == nblk - 1 and last
                    x = ops.graph_conv_cheby3(g, g2, x, cw, relu=relu, out=mesh_out if final else None)
        return x

    def meshnet(self, x):
        """[B, J, 5] -> [B, V0, 3] (Pose2Mesh.forward)"""
        b = x.shape[0]
        nblk = len(CL_F)
        li = 0
        for i in range(nblk):
            xin = x
            g = self.graphs[-(i + 1) + (1 if i == nblk - 1 else 0)]
            for _ in range(len(CL_F[i]) - 1):
                x = self._graph_conv(x, self.cl[li], g)
                li += 1
            if i == 0:
                x = self._linear(x.reshape(b, 1, 1, -1), self.fc).view(b, self.graphs[-2].v, CL_F[1][0])
            elif i < nblk - 2:
                x = ops.feat_interp_add(xin.contiguous(), x.contiguous(), up=2)
            elif i == nblk - 2:
                x = ops.feat_interp_add(xin.contiguous(), x.contiguous(), up=1)
        return x

    @ops.device_guarded
    def graphed(self, pose2d):
        """hipGraph replay for a fixed batch size (the forward is 26 short launches, i.e. launch-bound):
        returns (run, static_input, (mesh, pose3d)); copy new joints into static_input and call run()."""
        key = tuple(pose2d.shape)
        if key not in self._graphs:
            with torch.inference_mode(False), torch.no_grad():
                s_in = torch.empty_like(pose2d, dtype=torch.float32)
                s_in.copy_(pose2d)
                g, out = ops.capture_step(lambda: self.forward(s_in))
                self._graphs[key] = (g, s_in, out)
        g, s_in, out = self._graphs[key]
        return g.replay, s_in, out

    @ops.device_guarded
    def forward(self, pose2d, mesh_out=None):
        """pose2d [B,J,2] fp32 on the GPU -> (cam_mesh [B,V0,3], pose3d [B,J,3]), both on the GPU.  mesh_out: optional
        contiguous fp32 [B,V0,3] the mesh is written into (and returned)."""
        if pose2d.dim() != 3 or pose2d.shape[1:] != (self.num_joint, 2):
            raise ValueError(f"expected [B,{self.num_joint},2]")
        if not pose2d.is_cuda:
            raise RuntimeError("Pose2MeshEngine needs GPU tensors (no CPU fallback)")
        pose2d = pose2d.float().contiguous()
        b = pose2d.shape[0]
        pose3d = self.posenet(pose2d.reshape(b, -1)).view(b, self.num_joint, 3)    # (a view of the padded [B, 64] rows)
        if self.fused and b <= self.FUSED_MAX_BATCH:
            return self.meshnet_fused(ops.lifter_combine(pose2d, pose3d, fpad=self.cl[0][1]), mesh_out), pose3d
        comb = torch.cat((pose2d, pose3d / 1000), dim=2)          # pose2mesh_net.py:20 (glue, 105 floats per sample)
        mesh = self.meshnet(comb)
        if mesh_out is not None:
            mesh_out.copy_(mesh.view(mesh_out.shape))
            mesh = mesh_out
        return mesh, pose3d
