// Drives kirag_amd/csrc/encoder_model.hpp without a device (tests/test_encoder_model_host.py).  stdin:
//   config HIDDEN LAYERS HEADS FF VOCAB MAX_POS TYPE_VOCAB      (first line)
//   setting NAME v0 v1 ...      tensor NAME NUMEL      finalize      pools
// stdout, one line per command: "setting NAME rc=R msg", "tensor NAME slot=S family=F layer=L expect=N rc=R msg", "finalize rc=R msg" or "finalize rc=0 plan ...",
// "pools rc=0 plan pool0=... pool5=..." (resolve_pool on the last finalized plan).
// The loader's bookkeeping of the library (encoder_weights.hpp: enc_load_weight, enc_finalize) is repeated here in its host-only part.
#include "../../kirag_amd/csrc/encoder_model.hpp"

#include <iostream>
#include <sstream>

using namespace kr::model;

static std::string plan_line(const ModelPlan& p) {
    std::ostringstream o;
    o << "family=" << (int)p.family << " pre_ln=" << p.pre_ln << " rms=" << p.rms << " pos=" << (int)p.pos << " pad_idx=" << p.pad_idx << " half_window=" << p.half_window
      << " ff=" << (int)p.ff << " ff_gated=" << p.ff_gated << " qkv=";
    for (const LayerPlan& l : p.layers) o << (int)l.qkv;
    o << " attn=";
    for (const LayerPlan& l : p.layers) o << (int)l.attn;
    o << " heads=";
    for (int h = 0; h < HEAD_COUNT; ++h) o << (p.head[h] ? 1 : 0);
    o << " classifier=" << p.classifier << " classify_mean=" << p.classify_mean << " out_dim=" << p.out_dim << " out_width=" << p.out_width << " ws=" << p.ws
      << " zero_fill=" << p.zero_fill.size();
    return o.str();
}

int main() {
    kr_bert_cfg cfg{};
    std::string line, cmd, name;
    if (!std::getline(std::cin, line)) return 2;
    {
        std::istringstream in(line);
        if (!(in >> cmd >> cfg.hidden >> cfg.layers >> cfg.heads >> cfg.intermediate >> cfg.vocab >> cfg.max_pos >> cfg.type_vocab) || cmd != "config") return 2;
    }
    Settings set;
    Loaded ld(cfg.layers);
    bool finalized_once = false;
    ModelPlan plan;      // of the last finalize that succeeded
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "finalize") {
            ModelPlan p;
            const Error e = describe(cfg, set, ld, p);
            if (e.code) std::cout << "finalize rc=" << e.code << " " << e.msg << "\n";
            else std::cout << "finalize rc=0 plan " << plan_line(p) << "\n";
            if (!e.code) plan = p;
            finalized_once = finalized_once || e.code == 0;
            continue;
        }
        if (cmd == "pools") {      // resolve_pool of the finalized plan: poolN=pack,select,classify,score,splade,one_row for every KR_POOL_*
            if (!finalized_once) { std::cout << "pools rc=" << KR_ESTATE << " no finalized plan\n"; continue; }
            std::cout << "pools rc=0 plan";
            for (int pool : {KR_POOL_MEAN, KR_POOL_CLS, KR_POOL_CLASSIFY, KR_POOL_SPLADE, KR_POOL_LAST}) {
                const ForwardPool f = resolve_pool(plan, pool);
                std::cout << " pool" << pool << "=" << f.pack << "," << f.select << "," << f.classify << "," << f.score << "," << f.splade << "," << f.one_row;
            }
            std::cout << "\n";
            continue;
        }
        if (!(in >> name)) return 2;
        if (cmd == "setting") {
            std::vector<float> v;
            for (float x; in >> x;) v.push_back(x);
            bool stored = false;
            const Error e = set_setting(cfg, set, ld.heads, finalized_once, name.c_str(), v.data(), (int64_t)v.size(), stored);
            std::cout << "setting " << name << " rc=" << e.code << " " << e.msg << "\n";
        } else if (cmd == "tensor") {
            long long numel = 0;
            if (!(in >> numel)) return 2;
            int head = 0, idx = 0;
            if (find_head_tensor(name.c_str(), head, idx)) {
                int dim = 0;
                const Error e = check_head_tensor(cfg, head, idx, numel, ld.heads[head], finalized_once, dim);
                if (!e.code) { ld.heads[head].dim = dim; ld.heads[head].got |= 1u << idx; }
                std::cout << "tensor " << name << " head=" << head << " index=" << idx << " dim=" << dim << " rc=" << e.code << " " << e.msg << "\n";
                continue;
            }
            Resolved r;
            Error e = resolve_name(cfg, name.c_str(), r);
            if (!e.code) e = check_tensor(cfg, name.c_str(), r, numel, ld, finalized_once);
            if (!e.code) mark_loaded(ld, r);
            std::cout << "tensor " << name << " slot=" << r.slot << " family=" << (int)r.fam << " layer=" << r.layer << " expect=" << r.numel << " rc=" << e.code << " " << e.msg << "\n";
        } else {
            return 2;
        }
    }
    return 0;
}
