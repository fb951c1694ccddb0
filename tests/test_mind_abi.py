"""Host checks of the MIND entry points (csrc/mind_ops.hip): they return before any launch, so they are called here without a
GPU, with dummy non-null pointer values that nothing may dereference."""
import ctypes as C
import os

NEW = ["rec_mind_label_attn_bwd", "rec_mind_label_attn_fwd", "rec_mind_routing_bwd", "rec_mind_routing_fwd", "rec_mind_ssm_head"]


def _p(v):
    return None if v is None else C.c_void_p(v)


def _rfwd(L, batch=4, T=6, K=3, H=12, iters=3, ld_low=0, low=4096, seq=8192, logits=12288, W=16384, Z=20480, caps=24576):
    return L.rec_mind_routing_fwd(batch, T, K, H, iters, _p(low), ld_low, _p(seq), _p(logits), _p(W), _p(Z), _p(caps), None)


def _rbwd(L, batch=4, T=6, K=3, H=12, ld_dlow=0, d_caps=4096, Z=8192, W=12288, d_low=16384):
    return L.rec_mind_routing_bwd(batch, T, K, H, _p(d_caps), _p(Z), _p(W), _p(d_low), ld_dlow, None)


def _afwd(L, batch=4, K=3, H=12, pow_p=1.0, ld_caps=0, ld_target=0, ld_user=0, caps2=4096, target=8192, user=12288, attn=16384):
    return L.rec_mind_label_attn_fwd(batch, K, H, pow_p, _p(caps2), ld_caps, _p(target), ld_target, _p(user), ld_user, _p(attn), None)


def _abwd(L, batch=4, K=3, H=12, pow_p=1.0, ld_caps=0, ld_target=0, ld_duser=0, ld_dcaps=0, ld_dtarget=0, caps2=4096,
          target=8192, attn=12288, d_user=16384, d_caps2=20480, d_target=24576):
    return L.rec_mind_label_attn_bwd(batch, K, H, pow_p, _p(caps2), ld_caps, _p(target), ld_target, _p(attn), _p(d_user),
                                     ld_duser, _p(d_caps2), ld_dcaps, _p(d_target), ld_dtarget, None)


HEAD_PTRS = ("user", "true_w", "true_b", "S", "sample_b", "labels", "neg", "logq_true", "logq_neg", "loss", "d_true")


def _head(L, batch=4, H=12, n=6, ld_user=0, ld_true=0, ld_s=0, ld_dtw=0, ld_du0=0, d_true_w=49152, d_user0=53248, **ptr):
    v = {name: ptr.get(name, 4096 * (i + 1)) for i, name in enumerate(HEAD_PTRS)}
    return L.rec_mind_ssm_head(batch, H, n, _p(v["user"]), ld_user, _p(v["true_w"]), ld_true, _p(v["true_b"]), _p(v["S"]), ld_s,
                               _p(v["sample_b"]), _p(v["labels"]), _p(v["neg"]), _p(v["logq_true"]), _p(v["logq_neg"]), 0.25,
                               _p(v["loss"]), _p(v["d_true"]), _p(d_true_w), ld_dtw, _p(d_user0), ld_du0, None)


def _refused(L, fn, cases, name):
    for kw, word in cases:
        assert fn(L, **kw) == -1, kw
        assert word in L.rec_last_error() and name in L.rec_last_error(), (kw, L.rec_last_error())


SIZES = ((dict(T=0), b"seq_len_max"), (dict(T=65), b"seq_len_max"), (dict(K=0), b"k_max"), (dict(K=9), b"k_max"),
         (dict(H=0), b"hidden"), (dict(H=129), b"hidden"), (dict(batch=-1), b"batch"))


def test_routing_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _rfwd, SIZES + ((dict(iters=0), b"iters"), (dict(iters=9), b"iters"), (dict(ld_low=11), b"below the packed width"),
                                (dict(low=None), b"null"), (dict(seq=None), b"null"), (dict(logits=None), b"null"),
                                (dict(W=None), b"null"), (dict(Z=None), b"null"), (dict(caps=None), b"null")), b"rec_mind_routing_fwd")
    _refused(L, _rbwd, SIZES + ((dict(ld_dlow=11), b"below the packed width"), (dict(d_caps=None), b"null"), (dict(Z=None), b"null"),
                                (dict(W=None), b"null"), (dict(d_low=None), b"null")), b"rec_mind_routing_bwd")
    none = dict(low=None, seq=None, logits=None, W=None, Z=None, caps=None)
    assert _rfwd(L, batch=0, **none) == 0 and _rbwd(L, batch=0, d_caps=None, Z=None, W=None, d_low=None) == 0
    assert _rfwd(L, batch=0, T=65) == -1 and _rfwd(L, batch=0, ld_low=11) == -1 and _rbwd(L, batch=0, ld_dlow=11) == -1
    assert _rfwd(L, batch=0, T=64, K=8, H=128, iters=8) == 0 and _rfwd(L, batch=0, T=1, K=1, H=1, iters=1) == 0     # the limits
    assert _rbwd(L, batch=0, T=64, K=8, H=128) == 0 and _rfwd(L, batch=0, ld_low=12) == 0 and _rfwd(L, batch=0, ld_low=16) == 0


def test_label_attention_refusals_without_gpu(engine_lib):
    L = engine_lib
    both = ((dict(K=0), b"k_max"), (dict(K=9), b"k_max"), (dict(H=0), b"hidden"), (dict(H=129), b"hidden"), (dict(batch=-1), b"batch"),
            (dict(ld_caps=11), b"below the packed width"), (dict(ld_target=11), b"below the packed width"),
            (dict(caps2=None), b"null"), (dict(target=None), b"null"), (dict(attn=None), b"null"))
    _refused(L, _afwd, both + ((dict(ld_user=11), b"below the packed width"), (dict(user=None), b"null")), b"rec_mind_label_attn_fwd")
    _refused(L, _abwd, both + ((dict(ld_duser=11), b"below the packed width"), (dict(ld_dcaps=11), b"below the packed width"),
                               (dict(ld_dtarget=11), b"below the packed width"), (dict(d_user=None), b"null"),
                               (dict(d_caps2=None), b"null"), (dict(d_target=None), b"null")), b"rec_mind_label_attn_bwd")
    assert _afwd(L, batch=0, caps2=None, target=None, user=None, attn=None) == 0
    assert _abwd(L, batch=0, caps2=None, target=None, attn=None, d_user=None, d_caps2=None, d_target=None) == 0
    assert _afwd(L, batch=0, K=9) == -1 and _abwd(L, batch=0, ld_dcaps=11) == -1
    assert _afwd(L, batch=0, K=8, H=128, pow_p=2.0) == 0 and _abwd(L, batch=0, K=1, H=1) == 0                       # the limits


def test_ssm_head_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = [(dict(batch=-1), b"bad batch"), (dict(H=0), b"hidden"), (dict(H=1025), b"hidden"), (dict(n=0), b"n_sample"),
             (dict(n=65537), b"n_sample"), (dict(ld_user=11), b"below the packed width"), (dict(ld_true=11), b"below the packed width"),
             (dict(ld_s=5), b"below the packed width"), (dict(ld_dtw=11), b"below the packed width"),
             (dict(ld_du0=11), b"below the packed width")]
    cases += [({name: None}, b"null") for name in HEAD_PTRS]
    _refused(L, _head, cases, b"rec_mind_ssm_head")
    assert _head(L, batch=0, d_true_w=None, d_user0=None, **dict.fromkeys(HEAD_PTRS)) == 0
    assert _head(L, batch=0, ld_s=5) == -1 and _head(L, batch=0, n=65537) == -1
    assert _head(L, batch=0, n=1024) == 0 and _head(L, batch=0, n=65536, H=1024) == 0 and _head(L, batch=0, n=1, H=1) == 0


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("rec_mind_"))
    assert names == NEW and not any(n.endswith("_bytes") for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recengine.h")).read()
    for n in NEW:
        decl = header[header.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "workspace" not in decl and decl.rstrip().endswith("void* stream)"), n            # no workspace; the stream is last
        assert "int %s_workspace_bytes" % n not in header and "int %s_bytes" % n not in header
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[n][1]), n                               # one ctypes entry per argument
    assert (_lib.REC_MIND_MAX_T, _lib.REC_MIND_MAX_K, _lib.REC_MIND_MAX_H, _lib.REC_MIND_MAX_ITERS) == (64, 8, 128, 8)
    assert (_lib.REC_MIND_HEAD_MAX_DIM, _lib.REC_MIND_MAX_NEG) == (1024, 65536)
    for name, value in (("REC_MIND_MAX_T", 64), ("REC_MIND_MAX_K", 8), ("REC_MIND_MAX_H", 128), ("REC_MIND_MAX_ITERS", 8),
                        ("REC_MIND_HEAD_MAX_DIM", 1024), ("REC_MIND_MAX_NEG", 65536)):
        assert "#define %s %d\n" % (name, value) in header
