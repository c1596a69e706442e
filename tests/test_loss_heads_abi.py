"""CPU: the dispatcher-visible surface of the three loss heads' six library ops (srfrd_amd/ops.py over
srfrd_amd/loss_heads.py): the schemas, character for character, and what the shared fakes return under FakeTensorMode.
No GPU and no library call: a fake only propagates shapes."""
import pytest

SCHEMAS = {
    "xent_fwd": "srfrd::xent_fwd(Tensor hidden, Tensor targets, Tensor table, SymInt model_key) -> Tensor[]",
    "xent_bwd": "srfrd::xent_bwd(Tensor hidden, Tensor targets, Tensor table, Tensor lse, Tensor d_token_loss, "
                "SymInt model_key) -> Tensor[]",
    "sxent_fwd": "srfrd::sxent_fwd(Tensor hidden, Tensor targets, Tensor negatives, Tensor? log_q, Tensor table, "
                 "bool remove_hits, SymInt model_key) -> Tensor[]",
    "sxent_bwd": "srfrd::sxent_bwd(Tensor hidden, Tensor targets, Tensor negatives, Tensor? log_q, Tensor table, "
                 "bool remove_hits, Tensor lse, Tensor d_token_loss, SymInt model_key) -> Tensor[]",
    "tneg_fwd": "srfrd::tneg_fwd(Tensor hidden, Tensor targets, Tensor negatives, Tensor? log_q, Tensor table, "
                "SymInt objective, float beta, bool remove_hits, SymInt model_key) -> Tensor[]",
    "tneg_bwd": "srfrd::tneg_bwd(Tensor hidden, Tensor targets, Tensor negatives, Tensor? log_q, Tensor table, "
                "SymInt objective, float beta, bool remove_hits, Tensor lse, Tensor d_token_loss, SymInt model_key) -> Tensor[]",
}
METHODS = {"xent": "full_catalog_loss", "sxent": "sampled_softmax_loss", "tneg": "token_negatives_loss"}


@pytest.mark.parametrize("op", list(SCHEMAS))
def test_schema_is_pinned(op):
    import torch
    import srfrd_amd  # noqa: F401
    from srfrd_amd import ops
    assert op in ops.OPS
    assert str(getattr(torch.ops.srfrd, op).default._schema) == SCHEMAS[op]


def _head_args(head, torch):
    """(the arguments between targets and table, the scalars of the forward op, other scalars for the backward op)"""
    if head == "xent":
        return (), (), ()
    if head == "sxent":
        return (torch.empty(5, dtype=torch.int64), None), (True,), (False,)
    return (torch.empty(3, 7, 5, dtype=torch.int64), None), (0, 1.0, True), (1, 0.5, False)


@pytest.mark.parametrize("head", list(METHODS))
def test_ops_registered_with_fake_impls(head):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import srfrd_amd
    from srfrd_amd import ops
    fwd, bwd = getattr(torch.ops.srfrd, head + "_fwd"), getattr(torch.ops.srfrd, head + "_bwd")
    assert head + "_fwd" in ops.OPS and head + "_bwd" in ops.OPS
    assert fwd.default._schema.name == f"srfrd::{head}_fwd" and bwd.default._schema.name == f"srfrd::{head}_bwd"
    assert hasattr(srfrd_amd.SASRec, METHODS[head])
    with FakeTensorMode():
        h = torch.empty(3, 7, 50)
        y = torch.empty(3, 7, dtype=torch.int64)
        table = torch.empty(101, 50)
        ids, scalars_f, scalars_b = _head_args(head, torch)
        tl, lse, stats = fwd(h, y, *ids, table, *scalars_f, 0)
        assert tl.shape == (3, 7) and lse.shape == (3, 7) and stats.shape == (2,)
        assert tl.dtype == torch.float32 and lse.dtype == torch.float32 and stats.dtype == torch.float32
        dh, de = bwd(h, y, *ids, table, *scalars_b, lse, tl, 0)
        assert dh.shape == h.shape and de.shape == table.shape
        assert dh.dtype == torch.float32 and de.dtype == torch.float32
