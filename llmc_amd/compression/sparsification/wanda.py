"""Wanda with llmc's operator surface (llmc/compression/sparsification/wanda.py:10-56): a weight's score is
|W[r, k]| * ||X[:, k]||_2 and every output row loses its lowest-scoring fraction; no retraining, no Hessian.

  scaler_row[k] = sum over all calibration tokens of fp32(x[t, k])^2 / n_sequences      (get_row_scale, wanda.py:16-31)
  metric        = |W| * sqrt(scaler_row)                                                 (wanda.py:46-48)
  per row, the int(K * sparsity) smallest metrics (stable sort: ties by lower column) become 0    (wanda.py:50-56)

Both run in HIP kernels (csrc/prune.hip through sparse_ops): the sums of squares are folded batch by batch into one fp32 [K]
buffer per hooked layer by `cache_input_hook` — no activation is kept — and the selection reads each weight once and writes it
once. weight.sparsity_type 'n:m' runs the Wanda paper's semi-structured mode: n of every m consecutive input channels.

Where this differs from the reference, and why:
  * wanda.py:45 reads only the FIRST captured batch, input_feat[input_name][0]. With the shipped config (calib.bs = -1) there is
    one batch and this is the same statistic; when the calibration data arrives in several batches ours uses all of them, as the
    method is defined: scaler_row = (sum over every batch) / (total number of sequences).
  * wanda.py:30 takes torch.norm(...) ** 2: a square root of the sum, squared again, two more roundings than the sum itself.
    Ours divides the sum. The selections agree except where two metrics of a row lie within those roundings of each other
    (tests/test_sparse_e2e_gpu.py bounds it); given the reference's own scaler_row the pruned weights are bit-identical
    (tests/golden/sparse.npz).
  * wanda.py:54 reads self.sparser.sparsity, which the reference never defines; the base class defines it here.
  * n_prune = int(K * sparsity) is Python's double arithmetic, the reference's own expression."""
import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import sparse_ops
from .base_blockwise_sparsification import BaseBlockwiseSparsification


class RowSums:
    """The running statistic of one hooked layer: acc = fp32 [K] sums of squares over every token seen, n = sequences seen,
    scaler_row = acc / n (kept current by the kernel that folds a batch)."""
    __slots__ = ('acc', 'scaler_row', 'n')

    def __init__(self):
        self.acc = self.scaler_row = None
        self.n = 0

    def add(self, act):
        if act.dim() == 2:
            act = act.unsqueeze(0)
        self.n += act.shape[0]
        self.acc, self.scaler_row = sparse_ops.col_sqsum(act, self.acc, init=self.acc is None, nsamples=self.n)


@ALGO_REGISTRY
class Wanda(BaseBlockwiseSparsification):
    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)
        if not hasattr(self, 'sparsity'):
            raise ValueError('Wanda needs sparse.weight.sparsity (or an n:m sparsity_type)')
        if self.data_free:
            raise ValueError('Wanda scores weights by the norms of their input channels: it needs calibration data')

    def cache_input_hook(self, m, x, y, name, feat_dict):
        """Fold the batch into the layer's running sums instead of keeping it (the reference appends every input to a list)."""
        st = feat_dict[name]
        if not isinstance(st, RowSums):
            st = feat_dict[name] = RowSums()
        st.add(x[0].detach())

    @torch.no_grad()
    def get_row_scale(self, layer, act):
        """The reference's statistic for a given `act` (wanda.py:16-31): sum over all its rows of x^2 per input channel, divided
        by act.shape[0] (a 2-D act counts as one sequence). -> fp32 [K] on the layer's device."""
        if len(act.shape) == 2:
            act = act.unsqueeze(0)
        nsamples = act.shape[0]
        act = act.to(layer.weight.device)
        return sparse_ops.col_sqsum(act.reshape((-1, act.shape[-1])), nsamples=nsamples)[1]

    def _scaler_row(self, layer, feat):
        if isinstance(feat, RowSums):
            return feat.scaler_row
        st = RowSums()          # the reference's protocol: a list of captured batches
        for act in feat:
            st.add(act.to(layer.weight.device))
        return st.scaler_row

    @torch.no_grad()
    def subset_transform(self, subset, input_feat, subset_kwargs):
        layers_dict = subset['layers']
        input_name = subset['input'][0]
        layers = list(layers_dict.values())
        scaler_row = None
        for layer in layers:
            if scaler_row is None:
                scaler_row = self._scaler_row(layer, input_feat[input_name])
            W = layer.weight.data
            if self.nm is not None:
                n, m = self.nm
                sparse_ops.prune_rows(W, scaler_row, n, m)
            else:
                sparse_ops.prune_rows(W, scaler_row, int(W.shape[1] * self.sparser.sparsity))
