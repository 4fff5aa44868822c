"""BERT encoder for the Parallax benchmark config.

Reference workload: examples/benchmark/bert.py (TF-model-garden BERT-large
pretraining). Implemented from the architecture (Devlin et al. 2018):
token/position/segment embeddings -> N transformer encoder layers ->
masked-LM head (weight-tied). BASELINE config #3 is BERT-base Parallax on
8x MI355X: dense params sync over bucketed RCCL all-reduce, the (sparse)
embedding tables go to load-balanced PS owners.

Attention runs the fused MFMA kernels (ops/fused_attention.py; torch SDPA
where they do not apply), hidden dropout + residual + LayerNorm and the
Linear bias gradients their HIP kernels, and the masked-LM loss the fused linear + cross-entropy kernels
(ops/fused_linear_ce.py), which compute only the labelled positions and
never store the logits. Params stay fp32 with bf16 autocast compute.
"""

import torch
import torch.nn as nn

from autodist_amd.ops.fused_linear import FusedLinear, fused_linear


class BertConfig:
    def __init__(self, vocab_size=30522, hidden=768, layers=12, heads=12,
                 intermediate=3072, max_seq=512, type_vocab=2, dropout=0.1,
                 max_predictions=None):
        # the data pipeline's max_predictions_per_seq; None: no bound. The
        # MLM loss uses it as ONE bound for the batch, not per sequence: of
        # the labelled positions of a batch, in input order, those past the
        # first batch * max_predictions are dropped (data that keeps to the
        # per-sequence bound never reaches it).
        self.max_predictions = max_predictions
        self.vocab_size = vocab_size
        self.hidden = hidden
        self.layers = layers
        self.heads = heads
        self.intermediate = intermediate
        self.max_seq = max_seq
        self.type_vocab = type_vocab
        self.dropout = dropout

    @classmethod
    def base(cls):
        return cls()

    @classmethod
    def large(cls):
        return cls(hidden=1024, layers=24, heads=16, intermediate=4096)

    @classmethod
    def tiny(cls):  # CI-sized
        return cls(vocab_size=1000, hidden=64, layers=2, heads=4,
                   intermediate=128, max_seq=64)


class BertSelfAttention(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        self.qkv = FusedLinear(cfg.hidden, 3 * cfg.hidden)
        self.out = FusedLinear(cfg.hidden, cfg.hidden)
        self.dropout = cfg.dropout

    def forward(self, x, attn_mask=None):
        B, S, H = x.shape
        qkv = self.qkv(x).view(B, S, 3, self.heads, self.head_dim)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        # serving path: the fused gfx950 MFMA attention kernel (falls back to
        # torch SDPA for training / masked / non-bf16 cases)
        from autodist_amd.ops.fused_attention import fused_sdpa
        o = fused_sdpa(q, k, v, attn_mask=attn_mask,
                       dropout_p=self.dropout if self.training else 0.0)
        o = o.transpose(1, 2).reshape(B, S, H)
        return self.out(o)


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        from autodist_amd.ops.fused_ln import FusedLayerNorm
        self.attn = BertSelfAttention(cfg)
        self.ln1 = FusedLayerNorm(cfg.hidden, eps=1e-12)
        self.fc1 = FusedLinear(cfg.hidden, cfg.intermediate)
        self.fc2 = FusedLinear(cfg.intermediate, cfg.hidden)
        self.ln2 = FusedLayerNorm(cfg.hidden, eps=1e-12)
        self.drop = nn.Dropout(cfg.dropout)

    def forward(self, x, attn_mask=None):
        # hidden dropout and residual adds fold into the fused bf16 LN
        # kernels (gfx950); self.drop only carries p
        p = self.drop.p
        x = self.ln1(self.attn(x, attn_mask), residual=x, dropout_p=p)
        h = self.fc2(torch.nn.functional.gelu(self.fc1(x)))
        return self.ln2(h, residual=x, dropout_p=p)


class BertModel(nn.Module):
    def __init__(self, cfg: BertConfig, sparse_embeddings=False):
        super().__init__()
        self.cfg = cfg
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.hidden,
                                    sparse=sparse_embeddings)
        self.pos_emb = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.seg_emb = nn.Embedding(cfg.type_vocab, cfg.hidden)
        from autodist_amd.ops.fused_ln import FusedLayerNorm
        self.emb_ln = FusedLayerNorm(cfg.hidden, eps=1e-12)
        self.emb_drop = nn.Dropout(cfg.dropout)
        self.layers = nn.ModuleList(BertLayer(cfg) for _ in range(cfg.layers))
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02)
        if isinstance(m, nn.Linear) and m.bias is not None:
            nn.init.zeros_(m.bias)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        B, S = input_ids.shape
        pos = torch.arange(S, device=input_ids.device).unsqueeze(0)
        seg = token_type_ids if token_type_ids is not None else \
            torch.zeros_like(input_ids)
        x = self.tok_emb(input_ids) + self.pos_emb(pos) + self.seg_emb(seg)
        x = self.emb_drop(self.emb_ln(x))
        mask = None
        if attention_mask is not None:
            mask = attention_mask[:, None, None, :].to(torch.bool)
        for layer in self.layers:
            x = layer(x, mask)
        return x


class BertForPreTraining(nn.Module):
    """MLM head (weight-tied to token embedding) + NSP head."""

    def __init__(self, cfg: BertConfig, sparse_embeddings=False):
        super().__init__()
        self.bert = BertModel(cfg, sparse_embeddings)
        from autodist_amd.ops.fused_ln import FusedLayerNorm
        self.mlm_dense = FusedLinear(cfg.hidden, cfg.hidden)
        self.mlm_ln = FusedLayerNorm(cfg.hidden, eps=1e-12)
        self.mlm_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.nsp = FusedLinear(cfg.hidden, 2)

    def _heads(self, input_ids, token_type_ids, attention_mask):
        """MLM transform output m [B, S, H] (the input of the tied output
        projection) and the NSP logits."""
        h = self.bert(input_ids, token_type_ids, attention_mask)
        m = self.mlm_ln(torch.nn.functional.gelu(self.mlm_dense(h)))
        return m, self.nsp(h[:, 0])

    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        m, nsp = self._heads(input_ids, token_type_ids, attention_mask)
        logits = fused_linear(m, self.bert.tok_emb.weight, self.mlm_bias)
        return logits, nsp

    def loss(self, input_ids, mlm_labels, nsp_labels=None,
             token_type_ids=None, attention_mask=None):
        from autodist_amd.ops.fused_linear_ce import (
            can_use_lce_kernels, fused_linear_cross_entropy)
        m, nsp = self._heads(input_ids, token_type_ids, attention_mask)
        table = self.bert.tok_emb.weight
        mp = self.bert.cfg.max_predictions
        if mp is not None or can_use_lce_kernels(m, table, self.mlm_bias):
            # the kernels: only the labelled positions, logits never stored.
            # With a bound set the op also serves the steps the kernels do
            # not (captured, fp32, CPU), by its torch composite, so every
            # step drops the same positions past the bound.
            l = fused_linear_cross_entropy(
                m, table, self.mlm_bias, mlm_labels,
                max_rows=None if mp is None else input_ids.size(0) * mp)
        else:
            logits = fused_linear(m, table, self.mlm_bias)
            l = torch.nn.functional.cross_entropy(
                logits.view(-1, logits.size(-1)), mlm_labels.view(-1),
                ignore_index=-100)
        if nsp_labels is not None:
            l = l + torch.nn.functional.cross_entropy(nsp, nsp_labels)
        return l


def bert_base(sparse_embeddings=False):
    return BertForPreTraining(BertConfig.base(), sparse_embeddings)


def bert_large(sparse_embeddings=False):
    return BertForPreTraining(BertConfig.large(), sparse_embeddings)


def bert_tiny(sparse_embeddings=False):
    return BertForPreTraining(BertConfig.tiny(), sparse_embeddings)
