"""LM1B LSTM language model for the PartitionedAR config.

Reference workload: examples/lm1b/{lm1b_train.py, language_model.py} — LSTM
LM on the One Billion Word benchmark, trained via `autodist.function`
(lm1b_train.py:62). Architecture: embedding -> multi-layer LSTM -> tied
softmax projection. BASELINE config #5 runs it with a simulator-selected
PartitionedAR strategy (the big embedding/softmax matrices split axis-0 into
per-shard all-reduce groups).
"""
import torch
import torch.nn as nn

from autodist_amd.ops.fused_lstm import can_use_fused_lstmp, fused_lstmp
from autodist_amd.ops.sampled_softmax import (LogUniformSampler,
                                              sampled_softmax_loss)


class LM1BModel(nn.Module):
    def __init__(self, vocab_size=793470, emb_dim=512, hidden=2048,
                 layers=2, proj=512, dropout=0.1, tie_weights=True,
                 sparse=False, sharded_softmax=False, num_sampled=0,
                 sampler_seed=0):
        super().__init__()
        self.sharded_softmax = sharded_softmax
        # num_sampled > 0: training uses the sampled softmax loss the
        # reference trains with (language_model.py: sampled_softmax_loss,
        # num_sampled = 8192); evaluation keeps the full softmax
        if num_sampled > 0 and sharded_softmax:
            raise ValueError("num_sampled > 0 with sharded_softmax=True: the "
                             "vocab-parallel sampled softmax is not built")
        self.num_sampled = num_sampled
        self.sampler = (LogUniformSampler(vocab_size, num_sampled,
                                          sampler_seed)
                        if num_sampled > 0 else None)
        if sharded_softmax:
            # vocab-parallel path (reference partitioner seam,
            # partitioner.py:577-602): row-sharded tied table — input
            # lookup over all-to-all, output projection + CE over the
            # 3-collective sharded softmax (parallel/vocab_parallel.py)
            from autodist_amd.parallel.sharded_embedding import \
                ShardedEmbedding
            from autodist_amd.parallel.vocab_parallel import \
                VocabParallelProjection
            assert tie_weights and proj == emb_dim
            self.emb = ShardedEmbedding(vocab_size, emb_dim)
            self.out = VocabParallelProjection(
                vocab_size, proj, bias=True, tied_shard=self.emb.shard,
                rank=self.emb.rank, world_size=self.emb.world_size,
                process_group=self.emb.process_group)
        else:
            self.emb = nn.Embedding(vocab_size, emb_dim, sparse=sparse)
            if tie_weights:
                assert proj == emb_dim
                self.out_weight = self.emb.weight
            else:
                self.out_weight = nn.Parameter(
                    torch.randn(vocab_size, proj) * 0.02)
            self.out_bias = nn.Parameter(torch.zeros(vocab_size))
            nn.init.normal_(self.emb.weight, std=0.02)
        self.lstm = nn.LSTM(emb_dim, hidden, num_layers=layers,
                            proj_size=proj, batch_first=True,
                            dropout=dropout if layers > 1 else 0.0)
        self.drop = nn.Dropout(dropout)

    def _hidden(self, tokens, state=None):
        x = self.drop(self.emb(tokens))
        # Under autocast on the GPU the LSTM runs on the fused bf16 LSTMP
        # kernels (ops/fused_lstm.py) where they serve this module. Otherwise
        # it runs OUTSIDE autocast in fp32: the decomposed ROCm LSTM
        # thrashes bf16<->fp32 casts around every pointwise op under
        # autocast (~170 cast kernels/step measured), so a clean fp32 pass
        # is faster and more precise than stock bf16.
        if torch.is_autocast_enabled() and x.is_cuda:
            if can_use_fused_lstmp(x, self.lstm):
                h, state = fused_lstmp(x, self.lstm, state)
            else:
                with torch.autocast(device_type="cuda", enabled=False):
                    h, state = self.lstm(x.float(), state)
        else:
            h, state = self.lstm(x, state)
        return self.drop(h), state

    def forward(self, tokens, state=None):
        h, state = self._hidden(tokens, state)
        if self.sharded_softmax:
            return self.out.full_logits(h), state
        logits = torch.nn.functional.linear(h, self.out_weight,
                                            self.out_bias)
        return logits, state

    def loss(self, tokens, targets, state=None):
        if self.sharded_softmax:
            h, _ = self._hidden(tokens, state)
            return self.out.loss(h, targets)
        if self.num_sampled > 0 and self.training:
            h, _ = self._hidden(tokens, state)
            h = h.reshape(-1, h.size(-1))
            targets = targets.reshape(-1)
            sampled, logq_samp = self.sampler.sample(h.device)
            return sampled_softmax_loss(
                h, self.out_weight, self.out_bias, targets, sampled,
                self.sampler.logq_true(targets), logq_samp,
                sparse_grad=self.emb.sparse)
        logits, _ = self.forward(tokens, state)
        return torch.nn.functional.cross_entropy(
            logits.reshape(-1, logits.size(-1)), targets.reshape(-1))


def lm1b_small(vocab_size=10000, **kw):
    kw.setdefault("emb_dim", 256)
    kw.setdefault("hidden", 512)
    kw.setdefault("proj", 256)
    return LM1BModel(vocab_size, **kw)


def lm1b_full(**kw):
    return LM1BModel(**kw)
