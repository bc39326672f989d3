"""Generate tests/golden/vqa_small.npz from the REFERENCE's own models/med.py (through oracle/ref_shim.py).

Run in the build container only (needs the reference tree and `transformers`):

    python tests/golden/make_vqa_golden.py [seed]      # vqa_small.npz
    python tests/golden/make_vqa_golden.py keys        # blip_vqa_keys.json
    python tests/golden/make_vqa_golden.py search      # first seed whose margins hold

Small geometry of the existing goldens (hidden 256, 4 heads, 2 layers, vocabulary 512) with the weights ALREADY committed:
the text encoder of med_itm_small.npz and the decoder of med_decoder_small.npz (its encoder width is 256, the hidden size).
The file written here holds inputs and expected outputs only.  The statements of models/blip_vqa.py:85-167 run literally on
token ids (BLIP_VQA.__init__ would fetch a tokenizer); the beam search of `generate` is oracle/beam_ref.py driven by the
reference decoder, as for the caption goldens.

SEED is chosen so that the reference's own decisions have margins the f16 path cannot cross (printed below): every question's
k-th / (k+1)-th first-token log-probability and best / second-best log_probs_sum are further apart than
1.25e-3 x logit scale x 2 x target tokens.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from common import load_golden  # noqa: E402
from oracle import beam_ref, ref_shim  # noqa: E402

SEED = 1
PAD, SEP, DEC, ENC = 0, 102, 510, 509
Q_LENS = [3, 9, 33, 35]
Q_IMAGE = [0, 1, 2, 0]
N_ANSWERS, K_TEST = 40, 8
PLAIN_F16_REL = 1.25e-3


def inputs(seed):
    rng = np.random.default_rng(seed)
    Tq = max(Q_LENS)
    q_ids = np.zeros((len(Q_LENS), Tq), dtype=np.int64)
    q_mask = np.zeros_like(q_ids)
    for i, n in enumerate(Q_LENS):
        q_ids[i, :n] = rng.integers(110, 500, size=n)
        q_ids[i, 0], q_ids[i, n - 1] = ENC, SEP
        q_mask[i, :n] = 1
    firsts = rng.permutation(np.arange(110, 500))[:N_ANSWERS]          # 40 distinct first tokens
    a_lens = rng.integers(3, 9, size=N_ANSWERS)                        # [DEC] .. [SEP]: 3..8 tokens
    a_lens[:6] = [3, 8, 4, 7, 5, 6]
    Ta = int(a_lens.max())
    a_ids = np.zeros((N_ANSWERS, Ta), dtype=np.int64)
    a_mask = np.zeros_like(a_ids)
    for i, n in enumerate(a_lens):
        a_ids[i, :n] = rng.integers(110, 500, size=n)
        a_ids[i, 0], a_ids[i, 1], a_ids[i, n - 1] = DEC, firsts[i], SEP
        a_mask[i, :n] = 1
    n_train = [2, 1, 3, 2]
    train_answers = rng.permutation(N_ANSWERS)[:sum(n_train)]
    weights = rng.uniform(0.2, 1.0, size=sum(n_train)).astype(np.float32)
    return dict(q_ids=q_ids, q_mask=q_mask, a_ids=a_ids, a_mask=a_mask, n_train=np.asarray(n_train),
                train_answers=train_answers, train_weights=weights)


def run(seed, verbose=True):
    _, med = ref_shim.load()
    sd_e, g_e = load_golden("med_itm_small.npz")
    sd_d, _ = load_golden("med_decoder_small.npz")
    cfg = ref_shim.med_config(encoder_width=256)
    cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size = 256, 4, 512
    cfg.num_hidden_layers, cfg.vocab_size, cfg.max_position_embeddings = 2, 512, 64
    text_encoder = med.BertModel(cfg, add_pooling_layer=False).eval()
    text_decoder = med.BertLMHeadModel(cfg).eval()
    for m, sd, p in ((text_encoder, sd_e, "text_encoder."), (text_decoder, sd_d, "text_decoder.")):
        msg = m.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)}, strict=False)
        assert all("position_ids" in k for k in msg.missing_keys) and not msg.unexpected_keys, msg
    d = inputs(seed)
    enc = torch.from_numpy(g_e["enc"])                                  # [3, 17, 256]
    image_embeds = enc[torch.tensor(Q_IMAGE)]
    image_atts = torch.ones(image_embeds.size()[:-1], dtype=torch.long)
    q_ids, q_mask = torch.from_numpy(d["q_ids"]), torch.from_numpy(d["q_mask"])
    a_ids, a_mask = torch.from_numpy(d["a_ids"]), torch.from_numpy(d["a_mask"])
    k = K_TEST
    with torch.no_grad():
        # ---- models/blip_vqa.py:85-89
        question_output = text_encoder(q_ids, attention_mask=q_mask, encoder_hidden_states=image_embeds,
                                       encoder_attention_mask=image_atts, return_dict=True)
        states = question_output.last_hidden_state
        # ---- :91-105 (generate; the search itself is oracle/beam_ref.py)
        num_beams = 3
        question_states = states.repeat_interleave(num_beams, dim=0)
        question_atts = torch.ones(question_states.size()[:-1], dtype=torch.long)
        trace = []

        def step(ids, beam_idx):
            t = torch.from_numpy(ids)
            o = text_decoder(t, attention_mask=torch.ones_like(t), encoder_hidden_states=question_states,
                             encoder_attention_mask=question_atts, return_dict=True, is_decoder=True)
            return o.logits[:, -1].numpy()

        bos_ids = np.full((len(Q_LENS), 1), DEC, dtype=np.int64)
        seqs, _ = beam_ref.beam_search(step, bos_ids, num_beams=num_beams, max_length=10, min_length=1, eos_token_id=SEP,
                                       pad_token_id=PAD, trace=trace)
        gen = np.full((len(Q_LENS), 10), PAD, dtype=np.int64)
        for b, s in enumerate(seqs):
            gen[b, :len(s)] = s
        # smallest gap between adjacent candidates of a question over its search: a near-tie may flip on the device
        gen_gap = np.min([np.min(t["cand_scores"][:, :-1] - t["cand_scores"][:, 1:], axis=1) for t in trace], axis=0)
        # ---- :120-167 (rank_answer)
        num_ques = states.size(0)
        start_ids = a_ids[0, 0].repeat(num_ques, 1)
        start_output = text_decoder(start_ids, encoder_hidden_states=states, encoder_attention_mask=q_mask, return_dict=True,
                                    reduction="none")
        logits = start_output.logits[:, 0, :]
        answer_first_token = a_ids[:, 1]
        prob_first_token = F.softmax(logits, dim=1).index_select(dim=1, index=answer_first_token)
        topk_probs, topk_ids = prob_first_token.topk(k, dim=1)
        input_ids, input_atts = [], []
        for b, topk_id in enumerate(topk_ids):
            input_ids.append(a_ids.index_select(dim=0, index=topk_id))
            input_atts.append(a_mask.index_select(dim=0, index=topk_id))
        input_ids = torch.cat(input_ids, dim=0)
        input_atts = torch.cat(input_atts, dim=0)
        targets_ids = input_ids.masked_fill(input_ids == PAD, -100)
        question_states2 = states.repeat_interleave(k, dim=0)      # (each question's states and mask k times, question-major)
        question_atts2 = q_mask.repeat_interleave(k, dim=0)
        output = text_decoder(input_ids, attention_mask=input_atts, encoder_hidden_states=question_states2,
                              encoder_attention_mask=question_atts2, labels=targets_ids, return_dict=True, reduction="none")
        log_probs_sum = -output.loss
        log_probs_sum = log_probs_sum.view(num_ques, k)
        max_topk_ids = log_probs_sum.argmax(dim=1)
        max_ids = topk_ids[max_topk_ids >= 0, max_topk_ids]
        # ---- :51-79 (train=True)
        n = d["n_train"].tolist()
        t_ids, t_mask = a_ids[torch.from_numpy(d["train_answers"])], a_mask[torch.from_numpy(d["train_answers"])]
        answer_targets = t_ids.masked_fill(t_ids == PAD, -100)
        qs, qa = [], []
        for b, nb in enumerate(n):
            qs += [states[b]] * nb
            qa += [q_mask[b]] * nb
        answer_output = text_decoder(t_ids, attention_mask=t_mask, encoder_hidden_states=torch.stack(qs, 0),
                                     encoder_attention_mask=torch.stack(qa, 0), labels=answer_targets, return_dict=True,
                                     reduction="none")
        loss = (torch.from_numpy(d["train_weights"]) * answer_output.loss).sum() / len(Q_LENS)
    # ---- the oracle's own margins against what f16 operands may move
    scale = max(1.0, logits.abs().max().item())
    g = PLAIN_F16_REL * scale
    lp = torch.log_softmax(logits.double(), 1).index_select(1, answer_first_token)
    srt = lp.sort(dim=1, descending=True).values
    gap1 = (srt[:, k - 1] - srt[:, k]).numpy()
    n_tgt = (a_mask.sum(1) - 1)
    s2 = log_probs_sum.double().sort(dim=1, descending=True)
    gap2 = (s2.values[:, 0] - s2.values[:, 1]).numpy()
    nt = n_tgt[topk_ids.gather(1, s2.indices[:, :2])].max(dim=1).values.numpy()
    ok = bool((gap1 > 2 * g).all() and (gap2 > 2 * g * nt).all())
    ties = int((prob_first_token.sort(dim=1).values.diff(dim=1) == 0).sum())
    if verbose:
        print(f"seed {seed}: logit scale {scale:.3f}, f16 gate {g:.3e}; stage-1 gaps {gap1} (need > {2 * g:.3e}); stage-2 gaps {gap2} "
              f"(need > {2 * g * nt}); generate gaps {gen_gap}; exact stage-1 ties {ties}; margins hold: {ok}")
    out = dict(seed=np.asarray(seed), enc=g_e["enc"], q_image=np.asarray(Q_IMAGE), k=np.asarray(k), **d,
               question_states=states.numpy(), first_logits=logits.numpy(), topk_ids=topk_ids.numpy(),
               log_probs_sum=log_probs_sum.numpy(), max_ids=max_ids.numpy(), gen_ids=gen, gen_gap=gen_gap.astype(np.float32),
               train_loss=np.asarray(loss.item(), dtype=np.float32), train_losses=answer_output.loss.numpy())
    return ok and ties == 0, out


def write_keys():
    """blip_vqa_keys.json: the state-dict key names of the reference's BLIP_VQA members (models/blip_vqa.py:26-34) at full size."""
    import json

    vit_mod, med = ref_shim.load()
    vit = vit_mod.VisionTransformer(img_size=480, patch_size=16, embed_dim=768, depth=12, num_heads=12, use_grad_checkpointing=False,
                                    ckpt_layer=0, drop_path_rate=0.1)
    enc = med.BertModel(config=ref_shim.med_config(encoder_width=768), add_pooling_layer=False)
    dec = med.BertLMHeadModel(config=ref_shim.med_config(encoder_width=768))
    keys = sorted([f"visual_encoder.{k}" for k in vit.state_dict()] + [f"text_encoder.{k}" for k in enc.state_dict()]
                  + [f"text_decoder.{k}" for k in dec.state_dict()])
    with open(os.path.join(HERE, "blip_vqa_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print(f"blip_vqa_keys.json: {len(keys)} names")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "keys":
        return write_keys()
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        for seed in range(64):
            ok, _ = run(seed)
            if ok:
                print("first seed whose margins hold:", seed)
                break
        return
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    ok, out = run(seed)
    assert ok, "the oracle's margins do not keep all four questions in for f16: pick another seed (`search`)"
    path = os.path.join(HERE, "vqa_small.npz")
    np.savez_compressed(path, **out)
    print(f"vqa_small.npz: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
