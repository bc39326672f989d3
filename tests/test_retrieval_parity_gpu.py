"""The BLIP retrieval backend (--encoder_version blip) in the parity precision mode (packing.set_parity_mode(True, model)): ITC
embeddings and re-rank scores against the fp32 restatement (oracle/retrieval_ref.py), the per-frame visual tokens of
BlipVisualTokenizer rank by rank against the reference form, the [CLS]-only last layer of the compensated pair stack against the
all-token one, and the defaults ($VIDIL_PARITY leaves a BLIP_Retrieval plain)."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import perturb_, synthetic_frames

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def parity_retrieval():
    """Full-size BLIP_Retrieval (ViT-B/16 @ 224, 12-layer text encoder), perturbed random init with the ITC projections and the
    ITM head scaled up so that similarities and re-rank logits spread like a trained model's; parity mode, f16 operands."""
    from vidil_amd.blip_retrieval import BLIP_Retrieval
    from vidil_amd.packing import set_compute_dtype, set_parity_mode
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    torch.manual_seed(0)
    m = BLIP_Retrieval(image_size=224, vit="base", tokenizer=SyntheticBertTokenizer()).eval()
    perturb_(m, 103)
    with torch.no_grad():
        m.vision_proj.weight.mul_(8); m.text_proj.weight.mul_(8); m.itm_head.weight.mul_(20)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    set_compute_dtype("f16", m)
    set_parity_mode(True, m)
    return m, sd


def _texts(sizes):
    """Class strings of 1 - 4 words per category, distinct token sequences (the synthetic tokenizer maps "w<id>" to token id; its
    first word is unique within the category; prompted: 6 - 9 tokens, so every batch carries padded captions)."""
    from vidil_amd.visual_tokenization import CATEGORIES

    return {key: [f"w{1000 + 5000 * c + i}" + "".join(f" w{1000 + (7919 * i + 104729 * j) % 29000}" for j in range(1, 1 + i % 4))
                  for i in range(n)]
            for c, (key, n) in enumerate(zip(CATEGORIES, sizes))}


def _oracle_text(m, sd, prompted):
    """retrieval_ref.text_features on the prompted strings (padding columns past the longest caption cut: masked keys) and the
    ids with [ENC] first / the mask the re-rank oracle takes."""
    from oracle import retrieval_ref

    ids, lens = m.tokenize(prompted)
    t = int(lens.max())
    ids, mask = ids[:, :t].long(), (torch.arange(t)[None] < lens[:, None]).long()
    with torch.no_grad():
        emb = torch.cat([retrieval_ref.text_features(sd, ids[i:i + 1024], mask[i:i + 1024]) for i in range(0, len(prompted), 1024)])
    ids_enc = ids.clone()
    ids_enc[:, 0] = m.tokenizer.enc_token_id
    return emb, ids_enc, mask


def _score_matrix(sd, y, img, txt, ids_enc, mask, k_test):
    """retrieval_ref.score_matrix with the frame's image tokens broadcast over the k_test pairs instead of repeated (the cross
    K / V of one frame projected once, not k_test times; test_oracle_broadcast_equals_score_matrix pins the two together)."""
    from oracle import med_ref

    sims = img @ txt.t()
    score = torch.full_like(sims, -100.0)
    for i in range(sims.shape[0]):
        topk_sim, topk_idx = sims[i].topk(k=k_test, dim=0)
        h, _ = med_ref.bert_model(sd, "text_encoder.", ids_enc[topk_idx], mask[topk_idx], enc=y[i:i + 1], is_decoder=False)
        score[i, topk_idx] = F.linear(h[:, 0, :], sd["itm_head.weight"], sd["itm_head.bias"])[:, 1] + topk_sim
    return sims, score


def test_oracle_broadcast_equals_score_matrix(parity_retrieval):
    from oracle import clip_ref, retrieval_ref

    m, sd = parity_retrieval
    x = clip_ref.preprocess_u8(synthetic_frames(1, 1, first_video=20)[0])
    txt_ref, ids_enc, mask = _oracle_text(m, sd, [f"A photo of {t}" for t in _texts((40,))["objects"]])
    with torch.no_grad():
        y, img = retrieval_ref.image_features(sd, x)
        s0, ref = retrieval_ref.score_matrix(sd, y, img, txt_ref, ids_enc, mask, 6)
        s1, got = _score_matrix(sd, y, img, txt_ref, ids_enc, mask, 6)
    assert torch.equal(s0, s1) and torch.equal(ref == -100.0, got == -100.0)
    assert (ref - got).abs().max().item() < 1e-5


def test_parity_itc_embeddings_vs_fp32_oracle(parity_retrieval):
    """image_features_u8 / image_features / text_features and BLIP_ITM.forward(match_head='itc') in the parity mode: within 3e-6
    of the fp32 restatement (the plain 16-bit path is asserted at 2e-3), unit norm to 1e-5."""
    from oracle import clip_ref, retrieval_ref
    from vidil_amd.blip_itm import BLIP_ITM

    m, sd = parity_retrieval
    u8 = synthetic_frames(1, 8, first_video=21)[0]
    x = clip_ref.preprocess_u8(u8)
    with torch.no_grad():
        _, img_ref = retrieval_ref.image_features(sd, x)
    y3, img = m.image_features_u8(torch.from_numpy(u8).to(DEV))
    assert y3.shape[1] == 3 * 768
    img = img.cpu()
    _, img_f32 = m.image_features(x.to(DEV))
    prompted = [f"A photo of {t}" for t in _texts((300,))["objects"]]
    txt_ref, ids_enc, _ = _oracle_text(m, sd, prompted)
    txt, ids, lens = m.text_features(prompted, DEV)
    txt = txt.cpu()
    assert torch.equal(ids.cpu()[:, :ids_enc.shape[1]].long(), ids_enc)
    e_img, e_f32, e_txt = ((img - img_ref).abs().max().item(), (img_f32.cpu() - img_ref).abs().max().item(),
                           (txt - txt_ref).abs().max().item())
    itc = BLIP_ITM.forward(m, x.to(DEV), prompted[:8], match_head="itc").cpu()
    e_itc = (itc - img_ref @ txt_ref[:8].t()).abs().max().item()
    e_fwd = (m(x.to(DEV), prompted[:8], match_head="itc").cpu() - img_ref @ txt_ref[:8].t()).abs().max().item()
    print(f"parity BLIP retrieval vs fp32 oracle: image embeds max|d| {e_img:.2e} (f32 entry {e_f32:.2e}), text embeds {e_txt:.2e}, "
          f"itc scores {e_itc:.2e} (BLIP_Retrieval.forward {e_fwd:.2e})  (plain 16-bit path: asserted 2e-3)")
    assert e_img < 3e-6 and e_f32 < 3e-6 and e_txt < 3e-6
    assert e_itc < 6e-6 and e_fwd < 6e-6
    assert (img.norm(dim=-1) - 1).abs().max().item() < 1e-5 and (txt.norm(dim=-1) - 1).abs().max().item() < 1e-5


def _all_token_itm(m, y3, n_images, ids, lens, group_start, max_group):
    """The parity ITM logits with every token through every layer (BertModel.encode): what itm_pairs computed before its
    [CLS]-only last layer."""
    from vidil_amd import kernels as K

    te = m.text_encoder
    p = m.packed()
    t = int(lens.max().item())
    ids = ids[:, :t].contiguous()
    cross = te.project_cross_kv(y3, n_images, y3.shape[0] // n_images)
    h32, _ = te.encode(ids, lens, cross, cross_groups=group_start, cross_max_group=max_group)
    P, C = ids.shape[0], te.config.hidden_size
    cls32 = h32.view(P, t, C)[:, 0].contiguous()
    a3 = K.split3(cls32, torch.empty((P, 3 * C), dtype=p["itm_w"].dtype, device=DEV))
    out = torch.empty((P, 2), dtype=torch.float32, device=DEV)
    K.gemm(a3, p["itm_w3"], p["itm_b"], out=out, split_k=True)
    return out


@pytest.mark.parametrize("kind", ["split", "f32"])
def test_parity_cls_only_last_layer_equals_the_all_token_layer(parity_retrieval, kind):
    """itm_pairs in the parity mode runs the last layer on the [CLS] rows only (BertModel.encode_cls_parity; its one-row
    self-attention is vidil_attention_f32's one-row-per-unit form for arith 1): same ITM logits as the all-token last layer to 2e-6
    of the logit scale, with padded captions, image-major groups of 70 and 128 pairs (> 32 query rows per image) and a pair_text
    expansion; and no farther from the fp32 oracle than the all-token logits.  (The two differ by fp32 summation order only: one
    softmax(q k^T) v row of either attention form is ~1e-6 from float64 at unit scale, ~1e-6 of this model's logit scale of ~13.)"""
    from oracle import clip_ref, med_ref, vit_ref
    from vidil_amd.packing import set_parity_attention

    m, sd = parity_retrieval
    set_parity_attention(kind, m)
    try:
        u8 = synthetic_frames(1, 3, first_video=22)[0]
        y3, _ = m.image_features_u8(torch.from_numpy(u8).to(DEV))
        prompted = [f"A photo of {t}" for t in _texts((128,))["objects"]]
        ids, lens = m.tokenize(prompted)
        ids[:, 0] = m.tokenizer.enc_token_id
        sizes = [128, 70, 128]
        g = torch.Generator().manual_seed(5)
        sel = torch.cat([torch.randperm(128, generator=g)[:n] for n in sizes])
        group_start = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32, device=DEV)
        d_ids, d_lens = ids[sel].to(DEV).contiguous(), lens[sel].to(DEV).contiguous()
        got = m.itm_pairs(y3, 3, d_ids, d_lens, group_start=group_start, max_group=128)
        ref = _all_token_itm(m, y3, 3, d_ids, d_lens, group_start, 128)
        via_text = m.itm_pairs(y3, 3, ids.to(DEV), lens.to(DEV), group_start=group_start, max_group=128, pair_text=sel.to(DEV))
        with torch.no_grad():
            y = vit_ref.vit_forward(sd, clip_ref.preprocess_u8(u8))
            t = int(lens.max())
            ids_o, mask_o = ids[:, :t].long(), (torch.arange(t)[None] < lens[:, None]).long()
            orc = []
            for f, n in enumerate(sizes):
                rows = sel[int(np.sum(sizes[:f])):int(np.sum(sizes[:f + 1]))]
                h, _ = med_ref.bert_model(sd, "text_encoder.", ids_o[rows], mask_o[rows], enc=y[f:f + 1], is_decoder=False)
                orc.append(F.linear(h[:, 0, :], sd["itm_head.weight"], sd["itm_head.bias"]))
            orc = torch.cat(orc)
        e = (got - ref).abs().max().item()
        scale = ref.abs().max().item()
        e_cls, e_all = (got.cpu() - orc).abs().max().item(), (ref.cpu() - orc).abs().max().item()
        print(f"parity ITM logits, [CLS]-only vs all-token last layer ({kind} attention): max|d| {e:.2e} (logit scale {scale:.2f}); "
              f"vs fp32 oracle: [CLS]-only {e_cls:.2e}, all-token {e_all:.2e}")
        assert e < 2e-6 * max(1.0, scale)
        assert e_cls <= 1.25 * e_all + 2e-6
        assert (via_text - got).abs().max().item() < 1e-6
        assert lens[sel].min() < lens[sel].max()                    # (padded captions in every launch)
    finally:
        set_parity_attention(None, m)


def test_parity_rerank_scores_and_visual_tokens_rank_by_rank(parity_retrieval):
    """BlipVisualTokenizer.process in the parity mode (224^2 frames, ViT-B/16, 2 videos x 8 frames, k_test 128, top-5, a few
    thousand texts per category) against the reference form on the fp32 oracle (retrieval_ref: image / text features, the per-frame
    score matrix of run_visual_tokenization.py:277-293, argsort): re-rank logits within the bound on the oracle's candidates, and
    every rank equal unless the oracle's own adjacent values are closer than 5e-6 (candidate membership: rank k_test vs
    k_test + 1 of the similarities) or twice the measured re-rank error (final order) — at most 5 % of ranks excluded."""
    from oracle import clip_ref, retrieval_ref
    from vidil_amd.packing import set_parity_mode
    from vidil_amd.visual_tokenization import CATEGORIES, BlipVisualTokenizer

    m, sd = parity_retrieval
    Nv, Fr, k_test, topk = 2, 8, 128, 5
    EXTRA = 4
    u8 = synthetic_frames(Nv, Fr, first_video=30)
    texts = _texts((3000, 2500, 1000, 2000))
    cfg = dict(topk_visualize=topk, k_test=k_test, image_size=224, prompt_version_visual_tokenization="v1")
    tok = BlipVisualTokenizer(cfg, m, texts, DEV)
    frames = torch.from_numpy(u8).to(DEV)
    out = tok.process([f"video{v}" for v in range(Nv)], frames, [[] for _ in range(Nv)])

    # ---- fp32 oracle: features, similarities, re-ranked score matrix per video and category
    oracle_txt = {}
    for key in CATEGORIES:
        oracle_txt[key] = _oracle_text(m, sd, [f"A photo of {t}" for t in texts[key]])
    err = 0.0
    per_frame = []
    for v in range(Nv):
        x = clip_ref.preprocess_u8(u8[v])
        with torch.no_grad():
            y, img = retrieval_ref.image_features(sd, x)
        y3, _ = m.image_features_u8(frames[v])
        for c, key in enumerate(CATEGORIES):
            txt_ref, ids_enc, mask = oracle_txt[key]
            with torch.no_grad():
                # (EXTRA candidates past rank k_test: the oracle's scores of the texts a near-tie at the k_test boundary could swap in)
                sims, full_x = _score_matrix(sd, y, img, txt_ref, ids_enc, mask, k_test + EXTRA)
            full = torch.full_like(full_x, -100.0)
            cand_x = sims.topk(k_test + EXTRA, dim=1).indices
            full.scatter_(1, cand_x[:, :k_test], torch.gather(full_x, 1, cand_x[:, :k_test]))
            # re-rank logits of the device on the oracle's candidates (itm + the oracle's sim) against the oracle's scores
            cand = sims.topk(k_test, dim=1).indices                                       # [F, k_test]
            rep = tok.text_repr[key]
            idx = cand.reshape(-1).to(DEV)
            gs = torch.arange(Fr + 1, dtype=torch.int32, device=DEV) * k_test
            itm = m.rerank(y3, Fr, rep["ids"][idx], rep["lens"][idx], gs, k_test).cpu().view(Fr, k_test)
            err = max(err, (itm + torch.gather(sims, 1, cand) - torch.gather(full, 1, cand)).abs().max().item())
            per_frame.append((v, key, sims.numpy(), full.numpy(), full_x.numpy()))
    RERANK_BOUND = 1.3e-4      # (the parity ITM bound of test_parity_mode_gpu.py is 2e-4; measured here: 6.3e-5)
    print(f"parity BLIP re-rank: logits vs fp32 oracle on its candidates max|d| {err:.2e} (asserted < {RERANK_BOUND:g})")
    assert err < RERANK_BOUND

    # ---- ranks
    GAP_SIM, gap = 5e-6, 2 * err
    ranks = m_member = m_order = 0
    for v, key, sims, full, full_x in per_frame:
        got = out[f"video{v}"]["frame_tokens"]
        for f in range(Fr):
            order = np.argsort(-full[f], kind="stable")[:topk + 1]
            top = full[f][order]
            # candidate membership: where the similarities at rank k_test / k_test + 1 are within GAP_SIM, the device may re-rank a
            # different boundary text; that can move the top-5 only if one of the texts within GAP_SIM of the boundary scores
            # within the final-order gap of the 5th best (the oracle's own score of each, from its EXTRA candidates)
            s_sorted = np.sort(sims[f])[::-1]
            band = np.flatnonzero((sims[f] >= s_sorted[k_test] - GAP_SIM) & (sims[f] <= s_sorted[k_test - 1] + GAP_SIM))
            member_clear = s_sorted[k_test - 1] - s_sorted[k_test] > GAP_SIM or (
                len(band) <= EXTRA + 1 and s_sorted[k_test + EXTRA - 1] < s_sorted[k_test] - GAP_SIM
                and np.all(full_x[f][band] < top[topk - 1] - gap))
            for r in range(topk):
                ranks += 1
                if not member_clear:
                    m_member += 1
                elif top[r] - top[r + 1] > gap and (r == 0 or top[r - 1] - top[r] > gap):
                    assert got[f][key][r] == texts[key][order[r]], (v, f, key, r, got[f][key], [texts[key][i] for i in order[:topk]])
                else:
                    m_order += 1
    masked = m_member + m_order
    print(f"parity BLIP e2e visual tokens: {ranks - masked}/{ranks} ranks compared exactly and equal ({masked} excluded: {m_member} "
          f"where a text within {GAP_SIM:g} of the rank-{k_test} similarity could enter the top-{topk}, {m_order} with a final-order "
          f"gap <= {gap:.1e})")
    assert masked <= 0.05 * ranks, (masked, ranks)

    # ---- cost of the parity backend against the plain one (same frames, same texts; tokenizer built per mode)
    def fps():
        frames_all = frames.reshape(-1, *frames.shape[2:])
        tok.frame_topk(frames_all)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            tok.frame_topk(frames_all)
        torch.cuda.synchronize()
        return 2 * frames_all.shape[0] / (time.perf_counter() - t0)

    f_par = fps()
    set_parity_mode(False, m)
    try:
        tok = BlipVisualTokenizer(cfg, m, texts, DEV)
        f_plain = fps()
    finally:
        set_parity_mode(True, m)
    print(f"BLIP visual-token backend, {Nv * Fr} frames x 4 categories x k_test {k_test}: parity {f_par:.1f} frames/s, plain "
          f"{f_plain:.1f} frames/s (parity at {f_par / f_plain:.2f}x of plain)")


def test_blip_retrieval_defaults_unchanged_under_env_parity():
    """The process-wide parity default ($VIDIL_PARITY=1 sets it at import) leaves a freshly built BLIP_Retrieval plain — outputs
    bitwise equal to a build without it; only an explicit per-model call switches it; fp8 is refused for the mode."""
    from vidil_amd import packing
    from vidil_amd.blip_retrieval import BLIP_Retrieval
    from vidil_amd.packing import set_compute_dtype, set_parity_mode
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    u8 = torch.from_numpy(synthetic_frames(1, 3, first_video=40)[0]).to(DEV)
    prompted = [f"A photo of w{100 + i}" + " w7" * (i % 3) for i in range(40)]

    def build():
        torch.manual_seed(1)
        m = BLIP_Retrieval(image_size=224, vit="base", tokenizer=SyntheticBertTokenizer()).eval()
        perturb_(m, 104)
        return m.to(DEV)

    def run(m):
        y16, img = m.image_features_u8(u8)
        txt, ids, lens = m.text_features(prompted, DEV)
        gs = torch.arange(4, dtype=torch.int32, device=DEV) * 8
        itm = m.rerank(y16, 3, ids[:24], lens[:24], gs, 8)
        return [y16, img, txt, itm]

    base = run(build())
    old = packing.parity_mode()
    set_parity_mode(True)                       # what $VIDIL_PARITY=1 selects
    try:
        m = build()
        assert not any(packing.parity_mode(s) for s in m.modules())
        got = run(m)
        assert all(torch.equal(a, b) for a, b in zip(base, got))
        set_parity_mode(True, m)
        y3, _ = m.image_features_u8(u8)
        assert y3.shape[1] == 3 * base[0].shape[1]
        set_compute_dtype("fp8", m)
        with pytest.raises(ValueError):
            m.image_features_u8(u8)
    finally:
        set_parity_mode(old)
