// Drives kirag_amd/csrc/encoder_model.hpp without a device the way the library's loader does, for the tail of a sentence-transformers pipeline
// (tests/test_st_pipeline_host.py): the settings config.normalize_output / config.pool_tokens / config.st_dense_activation and the head st_dense.*.  stdin:
//   config HIDDEN LAYERS HEADS FF VOCAB MAX_POS TYPE_VOCAB      (first line)
//   setting NAME v0 v1 ...      tensor NAME NUMEL      finalize
// stdout, one line per command: "setting NAME rc=R msg", "tensor NAME slot=S layer=L rc=R msg", "finalize rc=R msg" or
// "finalize rc=0 plan family=F heads=<one digit per head> out_dim=D out_width=W normalize=N pool_tokens=T st_tanh=A ws=X zero_fill=Z".
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
            std::cout << "finalize rc=0 plan family=" << (int)p.family << " heads=";
            for (int h = 0; h < HEAD_ALL; ++h) std::cout << (int)p.head[h];
            std::cout << " out_dim=" << p.out_dim << " out_width=" << p.out_width << " normalize=" << p.normalize << " pool_tokens=" << p.pool_tokens << " st_tanh=" << p.st_tanh
                      << " ws=" << p.ws << " zero_fill=" << p.zero_fill.size() << "\n";
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
