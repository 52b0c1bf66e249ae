// Drives kirag_amd/csrc/encoder_model.hpp without a device the way the library's loader does on a handle that may carry "config.head_dim"
// (tests/test_qwen3_host.py): check_tensor is given the setting's value, as enc_load_weight gives it.  stdin:
//   config HIDDEN LAYERS HEADS FF VOCAB MAX_POS TYPE_VOCAB      (first line)
//   setting NAME v0 v1 ...      tensor NAME NUMEL      finalize
// stdout, one line per command: "setting NAME rc=R msg", "tensor NAME slot=S layer=L rc=R msg", "finalize rc=R msg" or
// "finalize rc=0 plan family=F qkv=.. attn=.. kv_dim=A head_w=D q_dim=Dq qk_norm=N classifier=C out_width=W zero_fill=Z".
#include "../../kirag_amd/csrc/encoder_model.hpp"

#include <iostream>
#include <sstream>

using namespace kr::model;

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
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "finalize") {
            ModelPlan p;
            const Error e = describe(cfg, set, ld, p);
            if (e.code) { std::cout << "finalize rc=" << e.code << " " << e.msg << "\n"; continue; }
            std::cout << "finalize rc=0 plan family=" << (int)p.family << " qkv=";
            for (const LayerPlan& l : p.layers) std::cout << (int)l.qkv;
            std::cout << " attn=";
            for (const LayerPlan& l : p.layers) std::cout << (int)l.attn;
            std::cout << " kv_dim=" << p.kv_dim << " head_w=" << p.head_w << " q_dim=" << p.q_dim << " qk_norm=" << p.qk_norm << " classifier=" << p.classifier
                      << " out_width=" << p.out_width << " zero_fill=" << p.zero_fill.size() << "\n";
            finalized_once = true;
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
                std::cout << "tensor " << name << " slot=head layer=-1 rc=" << e.code << " " << e.msg << "\n";
                continue;
            }
            Resolved r;
            Error e = resolve_name(cfg, name.c_str(), r);
            if (!e.code) e = check_tensor(cfg, name.c_str(), r, numel, ld, finalized_once, set.value(SET_HEAD_DIM, 0));
            if (!e.code) mark_loaded(ld, r);
            std::cout << "tensor " << name << " slot=" << r.slot << " layer=" << r.layer << " rc=" << e.code << " " << e.msg << "\n";
        } else {
            return 2;
        }
    }
    return 0;
}
