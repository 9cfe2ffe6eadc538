// Parameter layout of the reference's state_dict inside the engine's flat arenas.
// Names and shapes follow src/models.py:652-698, transformers/modeling_bert.py:155-416 and
// src/char_cnn.py:9-75 exactly (427 keys for SpellBertPho2ResArch3).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/realise_hip.h"

namespace rl {

enum Arena { AR_TRAIN = 0, AR_UNUSED = 1, AR_FROZEN = 2, AR_BUF_F32 = 3, AR_BUF_I64 = 4, AR_COUNT = 5 };

struct TensorInfo {
  std::string name;
  int arena;
  int64_t offset;   // elements
  int ndim;
  int64_t shape[4];
  int64_t numel() const { int64_t n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }
};

struct LayerOff {      // offsets into AR_TRAIN
  int64_t qkv_w, qkv_b, ao_w, ao_b, ao_ln_g, ao_ln_b, in_w, in_b, out_w, out_b, out_ln_g, out_ln_b;
};
struct StackOff {
  int64_t word;        // AR_TRAIN offset, or -1 when the table is unused (inputs_embeds stacks)
  int64_t pos, type, ln_g, ln_b;
  std::vector<LayerOff> layers;
};
struct BnOff { int64_t g, b; int64_t rmean, rvar; int64_t nbt; };   // g,b: AR_TRAIN; rmean,rvar: AR_BUF_F32; nbt: AR_BUF_I64
struct BlockOff { int cin, cout; int64_t w1, w2, ws; BnOff bn1, bn2, bns; };

// The glyph tower as data (run.py:292 --image_model_type, models.py:681-686): every block is a BasicBlock with a stride-2 3x3
// convolution, a stride-1 3x3 convolution and a stride-2 1x1 shortcut, so a tower is its channel list; the map side halves per block.
//   type 0  CharResNet  (char_cnn.py:36-55): F -> 64 -> 128 -> 256 -> 512 -> 768, 32x32 -> 1x1, output [N, 768]
//   type 1  CharResNet1 (char_cnn.py:57-75): 1 -> 64 -> 128 -> 192 -> 192,        32x32 -> 2x2, output the NCHW flatten [N, 192 * 4]
static constexpr int TOWER_MAX_BLOCKS = 5;
struct Tower {
  int nblocks = 0;
  int chans[TOWER_MAX_BLOCKS + 1] = {0, 0, 0, 0, 0, 0};   // chans[0] = input channels, chans[k] = output channels of block k
  int top_side = 1;                                       // side of the last block's map
  int top_channels() const { return chans[nblocks]; }
  int top_pixels() const { return top_side * top_side; }
  int features() const { return top_channels() * top_pixels(); }       // width of the flattened output (char_cnn.py:54,74)
};
inline Tower tower_of(const realise_config& c) {
  Tower t;
  if (c.image_model_type == 1) { t.nblocks = 4; const int ch[5] = {1, 64, 128, 192, 192}; for (int i = 0; i < 5; ++i) t.chans[i] = ch[i]; }
  else { t.nblocks = 5; const int ch[6] = {c.num_fonts, 64, 128, 256, 512, 768}; for (int i = 0; i < 6; ++i) t.chans[i] = ch[i]; }
  t.top_side = c.glyph_size >> t.nblocks;
  return t;
}

struct Layout {
  std::vector<TensorInfo> tensors;
  int64_t arena_elems[AR_COUNT] = {0, 0, 0, 0, 0};
  std::vector<std::pair<int64_t, int64_t>> buckets;    // [begin, end) in AR_TRAIN, backward completion order
  StackOff bert, pho, outb;
  int64_t cls_w = -1, cls_b = -1;
  int64_t head_w = -1, head_b = -1, head_ln_g = -1, head_ln_b = -1;   // BertPredictionHeadTransform (Variant::mlm_head); cls_w / cls_b are then its decoder
  int64_t pho_emb = -1, gru_w_ih = -1, gru_w_hh = -1, gru_b_ih = -1, gru_b_hh = -1;
  int64_t res_ln_g = -1, res_ln_b = -1, gate_w = -1, gate_b = -1;
  int64_t int_w = -1, int_b = -1;                      // integrate [H, nsrc * H] + bias (Variant::concat), where gate_net sits on a gate model
  int64_t glyph = -1;                                  // AR_FROZEN
  Tower tower;                                         // nblocks == 0 without the glyph branch
  BlockOff blocks[TOWER_MAX_BLOCKS];
  int bert_groups = 0;                                 // number of buckets the bert layers are split in
};

inline int64_t align64(int64_t x) { return (x + 63) & ~(int64_t)63; }

// What a configuration computes.  Every layout / engine decision reads this, not model_type.
struct Variant {
  bool bert = true;      // the bert stack under a (tied or untied) classifier; false: the model starts at the pinyin branch
  bool arch = false;     // output_block behind a fusion of the branches
  bool pho = false;      // pinyin branch: pho_embeddings, pho_gru, pho_model
  bool res = false;      // glyph branch: glyph table, resnet, resnet_layernorm
  bool gate = false;     // gate fusion (gate_net); false on an arch model without concat: sum fusion
  int nsrc = 1;          // fusion sources: bert + the present branches
  bool gate_softmax = false;   // the gates are one softmax over the gate_net outputs (models.py:1143-1144), not sigmoids
  bool concat = false;         // the fusion is integrate = nn.Linear(nsrc * H, H) over torch.cat of the branches (models.py:628-629, :228-229)
  bool mlm_head = false;       // the classifier is BertOnlyMLMHead (modeling_bert.py:419-462): cls.predictions.* (cls2. without bert), no classifier.*
};
// The models, one row per realise_config.model_type; variant_of and variant_valid below only read the row.  A new model is a row here
// (and one in realise_amd/config.py) plus engine code for whatever it computes that no row before it did.
enum Fuse { FUSE_NONE = -1, FUSE_GATE = 0, FUSE_SUM = 1, FUSE_CONCAT = 2 };      // the values of realise_config.fusion
enum States { STATES_NOTHING, STATES_BRANCHES, STATES_BRANCHES_FUSION };           // what the config must say about the model itself
struct ModelRow {
  bool bert, arch, pho, res; Fuse fuse;
  bool switches;         // with_pho / with_res / fusion are read (src/models_abla.py:37-45): they drop branches, turn the gate into the sum
  bool gate_softmax, mlm_head;
  bool one_font;         // the glyph table is nn.Embedding(vocab, 1024) viewed as [N, 1, 32, 32]: num_fonts == 1, glyph_size == 32
  bool untied_only;      // the decoder is the model's own (tie_cls_weight is a `pass`, models.py:915-917) or there is no word table to tie to
  States states;         // with_pho / with_res (and fusion) must equal the row's: another model's config with the number changed is refused
  int out_layers;        // hard-wired depth of output_block (models.py:546, :185); 0: the config's
};
static constexpr ModelRow MODEL_ROWS[] = {
  // bert  arch   pho    res    fuse         switch softmax mlm   1font  untied states                  out
  {true,  false, false, false, FUSE_NONE,   false, false, false, false, false, STATES_NOTHING,         0},   // 0 SpellBert
  {true,  true,  true,  true,  FUSE_GATE,   false, false, false, false, false, STATES_NOTHING,         0},   // 1 SpellBertPho2ResArch3
  {true,  true,  true,  true,  FUSE_GATE,   true,  false, false, false, false, STATES_NOTHING,         0},   // 2 ...Arch3Abla (models_abla.py:33-96)
  {true,  true,  true,  true,  FUSE_GATE,   false, true,  false, true,  false, STATES_NOTHING,         0},   // 3 ...Arch4 (models.py:1023-1170)
  {true,  true,  true,  true,  FUSE_GATE,   false, false, true,  true,  true,  STATES_NOTHING,         0},   // 4 ...Arch3MLM (models.py:874-1020)
  {false, false, true,  false, FUSE_NONE,   false, false, true,  false, true,  STATES_BRANCHES,        0},   // 5 Pho2Pretrain (models.py:1286-1347)
  {true,  true,  true,  true,  FUSE_CONCAT, false, false, false, true,  false, STATES_BRANCHES_FUSION, 2},   // 6 ...Arch2 (models.py:513-649)
  {true,  true,  true,  false, FUSE_CONCAT, false, false, false, false, false, STATES_BRANCHES_FUSION, 2},   // 7 SpellBertPho2 (models.py:163-249)
};
inline const ModelRow* model_row(const realise_config& c) {
  return c.model_type >= 0 && c.model_type < (int)(sizeof(MODEL_ROWS) / sizeof(MODEL_ROWS[0])) ? &MODEL_ROWS[c.model_type] : nullptr;
}
inline Variant variant_of(const realise_config& c) {
  Variant v;
  const ModelRow* r = model_row(c); if (!r) return v;
  v.bert = r->bert; v.arch = r->arch; v.gate_softmax = r->gate_softmax; v.mlm_head = r->mlm_head;
  v.pho = r->pho && (!r->switches || c.with_pho != 0);
  v.res = r->res && (!r->switches || c.with_res != 0);
  const Fuse f = r->switches && c.fusion != 0 ? FUSE_SUM : r->fuse;
  v.gate = f == FUSE_GATE; v.concat = f == FUSE_CONCAT;
  if (v.arch) v.nsrc = 1 + (v.pho ? 1 : 0) + (v.res ? 1 : 0);
  return v;
}
// The rules of the row, each applied only where the row states it: what it does not state is carried unchecked.  Where the switches
// are read they are in range, and the sum fusion has both branches (the reference's sum path adds None otherwise).
inline bool variant_valid(const realise_config& c) {
  const ModelRow* r = model_row(c); if (!r) return false;
  if (r->one_font && (c.num_fonts != 1 || c.glyph_size != 32)) return false;
  if (r->untied_only && c.tie_classifier != 0) return false;
  if (r->states != STATES_NOTHING && (c.with_pho != (int)r->pho || c.with_res != (int)r->res)) return false;
  if (r->states == STATES_BRANCHES_FUSION && c.fusion != (int)r->fuse) return false;
  if (r->out_layers != 0 && c.out_layers != r->out_layers) return false;
  if (!r->switches) return true;
  if ((c.with_pho != 0 && c.with_pho != 1) || (c.with_res != 0 && c.with_res != 1) || (c.fusion != 0 && c.fusion != 1)) return false;
  return c.fusion == 0 || (c.with_pho == 1 && c.with_res == 1);
}
// variant_valid + the glyph tower: image_model_type 0 / 1 only (models.py:681-686 raises NotImplementedError for anything else).
// CharResNet1 is built with in_channels = 1 whatever num_fonts is and flattens a [192, 2, 2] map, so with the glyph branch present
// type 1 needs one font, hidden == 768 and a 32x32 glyph; without the branch the field is carried and ignored, as in the reference.
inline bool config_ok(const realise_config& c) {
  if (!variant_valid(c)) return false;
  if (c.image_model_type != 0 && c.image_model_type != 1) return false;
  if (c.image_model_type == 1 && variant_of(c).res && (c.num_fonts != 1 || c.hidden != 768 || c.glyph_size != 32)) return false;
  return true;
}

inline Layout build_layout(const realise_config& c) {
  Layout L;
  const int64_t H = c.hidden, I = c.intermediate, V = c.vocab;
  auto add = [&](int arena, const std::string& name, std::initializer_list<int64_t> shape) -> int64_t {
    TensorInfo t;
    t.name = name; t.arena = arena; t.ndim = (int)shape.size();
    int k = 0;
    for (auto s : shape) t.shape[k++] = s;
    for (; k < 4; ++k) t.shape[k] = 1;
    t.offset = L.arena_elems[arena];
    L.arena_elems[arena] = align64(t.offset + (t.ndim == 0 ? 1 : t.numel()));
    L.tensors.push_back(t);
    return t.offset;
  };
  auto alias = [&](const std::string& name, int arena, int64_t offset, std::initializer_list<int64_t> shape) {
    TensorInfo t;
    t.name = name; t.arena = arena; t.ndim = (int)shape.size(); t.offset = offset;
    int k = 0;
    for (auto s : shape) t.shape[k++] = s;
    for (; k < 4; ++k) t.shape[k] = 1;
    L.tensors.push_back(t);
  };
  auto add_layer = [&](const std::string& p) -> LayerOff {
    LayerOff o;
    // q,k,v adjacent so the fused [3H,H] projection (and its gradient) is one contiguous matrix
    o.qkv_w = add(AR_TRAIN, p + "attention.self.query.weight", {H, H});
    add(AR_TRAIN, p + "attention.self.key.weight", {H, H});
    add(AR_TRAIN, p + "attention.self.value.weight", {H, H});
    o.qkv_b = add(AR_TRAIN, p + "attention.self.query.bias", {H});
    add(AR_TRAIN, p + "attention.self.key.bias", {H});
    add(AR_TRAIN, p + "attention.self.value.bias", {H});
    o.ao_w = add(AR_TRAIN, p + "attention.output.dense.weight", {H, H});
    o.ao_b = add(AR_TRAIN, p + "attention.output.dense.bias", {H});
    o.ao_ln_g = add(AR_TRAIN, p + "attention.output.LayerNorm.weight", {H});
    o.ao_ln_b = add(AR_TRAIN, p + "attention.output.LayerNorm.bias", {H});
    o.in_w = add(AR_TRAIN, p + "intermediate.dense.weight", {I, H});
    o.in_b = add(AR_TRAIN, p + "intermediate.dense.bias", {I});
    o.out_w = add(AR_TRAIN, p + "output.dense.weight", {H, I});
    o.out_b = add(AR_TRAIN, p + "output.dense.bias", {H});
    o.out_ln_g = add(AR_TRAIN, p + "output.LayerNorm.weight", {H});
    o.out_ln_b = add(AR_TRAIN, p + "output.LayerNorm.bias", {H});
    return o;
  };
  auto add_layers_desc = [&](StackOff& s, const std::string& prefix, int hi, int lo) {   // layers hi..lo descending
    for (int l = hi; l >= lo; --l) s.layers[l] = add_layer(prefix + "encoder.layer." + std::to_string(l) + ".");
  };
  auto add_emb = [&](StackOff& s, const std::string& prefix, bool word_used) {
    s.pos = add(AR_TRAIN, prefix + "embeddings.position_embeddings.weight", {c.max_pos, H});
    s.type = add(AR_TRAIN, prefix + "embeddings.token_type_embeddings.weight", {c.type_vocab, H});
    s.ln_g = add(AR_TRAIN, prefix + "embeddings.LayerNorm.weight", {H});
    s.ln_b = add(AR_TRAIN, prefix + "embeddings.LayerNorm.bias", {H});
    if (word_used) s.word = add(AR_TRAIN, prefix + "embeddings.word_embeddings.weight", {V, H});
    else { s.word = -1; add(AR_UNUSED, prefix + "embeddings.word_embeddings.weight", {V, H}); }
    add(AR_UNUSED, prefix + "pooler.dense.weight", {H, H});      // BertPooler output is dropped by every
    add(AR_UNUSED, prefix + "pooler.dense.bias", {H});           // caller on this path (modeling_bert.py:410-416)
  };
  auto close_bucket = [&](int64_t& begin) {
    L.buckets.push_back({begin, L.arena_elems[AR_TRAIN]});
    begin = L.arena_elems[AR_TRAIN];
  };
  auto add_bn = [&](const std::string& p, int64_t C) -> BnOff {
    BnOff b;
    b.g = add(AR_TRAIN, p + "weight", {C});
    b.b = add(AR_TRAIN, p + "bias", {C});
    b.rmean = add(AR_BUF_F32, p + "running_mean", {C});
    b.rvar = add(AR_BUF_F32, p + "running_var", {C});
    b.nbt = add(AR_BUF_I64, p + "num_batches_tracked", {});
    return b;
  };

  const Variant vr = variant_of(c);
  int64_t begin = 0;
  if (vr.bert) L.bert.layers.resize(c.bert_layers);
  // the pinyin branch: pho_model, GRU, pinyin embedding (one bucket)
  auto add_pho = [&]() {
    L.pho.layers.resize(c.pho_layers);
    add_layers_desc(L.pho, "pho_model.", c.pho_layers - 1, 0);
    add_emb(L.pho, "pho_model.", false);
    L.gru_w_hh = add(AR_TRAIN, "pho_gru.weight_hh_l0", {3 * H, H});
    L.gru_b_hh = add(AR_TRAIN, "pho_gru.bias_hh_l0", {3 * H});
    L.gru_w_ih = add(AR_TRAIN, "pho_gru.weight_ih_l0", {3 * H, H});
    L.gru_b_ih = add(AR_TRAIN, "pho_gru.bias_ih_l0", {3 * H});
    L.pho_emb = add(AR_TRAIN, "pho_embeddings.weight", {c.pho_vocab, H});
    close_bucket(begin);
  };
  // BertOnlyMLMHead (modeling_bert.py:419-462) in backward completion order: decoder bias and weight, the transform's LayerNorm, its dense
  auto add_mlm_head = [&](const std::string& p) {
    L.cls_b = add(AR_TRAIN, p + "predictions.bias", {V});
    L.cls_w = add(AR_TRAIN, p + "predictions.decoder.weight", {V, H});
    L.head_ln_g = add(AR_TRAIN, p + "predictions.transform.LayerNorm.weight", {H});
    L.head_ln_b = add(AR_TRAIN, p + "predictions.transform.LayerNorm.bias", {H});
    L.head_w = add(AR_TRAIN, p + "predictions.transform.dense.weight", {H, H});
    L.head_b = add(AR_TRAIN, p + "predictions.transform.dense.bias", {H});
  };
  if (!vr.bert) {
    // Pho2Pretrain (models.py:1286-1347): bucket 0 = the head `cls2`, bucket 1 = the pinyin branch.  num_hidden_layers is carried and
    // ignored (models.py:1302 hard-wires the 4 pho layers); no bert.*, classifier.* or cls.* keys.
    add_mlm_head("cls2.");
    close_bucket(begin);
    add_pho();
    return L;
  }
  // ---- bucket 0: classifier bias (+ untied weight), output_block
  if (vr.mlm_head) add_mlm_head("cls.");
  else {
    L.cls_b = add(AR_TRAIN, "classifier.bias", {V});
    if (!c.tie_classifier) L.cls_w = add(AR_TRAIN, "classifier.weight", {V, H});
  }
  if (vr.arch) {
    L.outb.layers.resize(c.out_layers);
    add_layers_desc(L.outb, "output_block.", c.out_layers - 1, 0);
    add_emb(L.outb, "output_block.", false);
    close_bucket(begin);
    // ---- bucket 1: gate [G, (G+1)H] (models_abla.py:86-87), resnet LN, glyph ResNet (last block first) - never empty: sum fusion has both branches
    if (vr.gate) {
      L.gate_w = add(AR_TRAIN, "gate_net.weight", {vr.nsrc, (vr.nsrc + 1) * H});
      L.gate_b = add(AR_TRAIN, "gate_net.bias", {vr.nsrc});
    }
    if (vr.concat) {      // models.py:544, :183 - where gate_net sits; alone in this bucket without the glyph branch
      L.int_w = add(AR_TRAIN, "integrate.weight", {H, vr.nsrc * H});
      L.int_b = add(AR_TRAIN, "integrate.bias", {H});
    }
    if (vr.res) {
      L.res_ln_g = add(AR_TRAIN, "resnet_layernorm.weight", {H});
      L.res_ln_b = add(AR_TRAIN, "resnet_layernorm.bias", {H});
      L.tower = tower_of(c);
      for (int b = L.tower.nblocks; b >= 1; --b) {
        BlockOff& k = L.blocks[b - 1];
        k.cin = L.tower.chans[b - 1]; k.cout = L.tower.chans[b];
        const std::string p = "resnet.res_block" + std::to_string(b) + ".";
        k.w2 = add(AR_TRAIN, p + "residual_function.3.weight", {k.cout, k.cout, 3, 3});
        k.bn2 = add_bn(p + "residual_function.4.", k.cout);
        k.ws = add(AR_TRAIN, p + "shortcut.0.weight", {k.cout, k.cin, 1, 1});
        k.bns = add_bn(p + "shortcut.1.", k.cout);
        k.w1 = add(AR_TRAIN, p + "residual_function.0.weight", {k.cout, k.cin, 3, 3});
        k.bn1 = add_bn(p + "residual_function.1.", k.cout);
      }
    }
    close_bucket(begin);
    // ---- bucket 2 (with the pinyin branch): pho_model, GRU, pinyin embedding
    if (vr.pho) add_pho();
    // models.py:674-679: one font -> nn.Embedding "char_images.weight" [V, 1024]; several -> Parameter [V, F, 32, 32].  Same bytes.
    if (vr.res) {
      if (c.num_fonts == 1) L.glyph = add(AR_FROZEN, "char_images.weight", {V, (int64_t)c.glyph_size * c.glyph_size});
      else L.glyph = add(AR_FROZEN, "char_images_multifonts", {V, c.num_fonts, c.glyph_size, c.glyph_size});
    }
  }
  // ---- bert layers in groups of <= 4 (one bucket each)
  {
    int hi = c.bert_layers - 1;
    L.bert_groups = 0;
    while (hi >= 0) {
      const int lo = hi - 3 > 0 ? hi - 3 : 0;
      add_layers_desc(L.bert, "bert.", hi, lo);
      close_bucket(begin);          // SpellBert: the first group's bucket also holds the classifier bias
      ++L.bert_groups;
      hi = lo - 1;
    }
  }
  // ---- last bucket: bert embeddings (word table last: its gradient is complete last)
  add_emb(L.bert, "bert.", true);
  close_bucket(begin);
  if (c.tie_classifier && !vr.mlm_head) {
    L.cls_w = L.bert.word;
    alias("classifier.weight", AR_TRAIN, L.bert.word, {V, H});
  }
  return L;
}

}  // namespace rl
